// An object's symmetries from its own surface (SPEC.md section 17; ossid_code_amd/symmetry.py): candidate rigid transforms
// are scored by how well they map a thinned sample of the surface (the queries) back onto a dense one (the targets).
//   ossid_sym_grid    the uniform cell grid over the targets (cell_grid.h's sizing, a counting sort in global memory as
//                     ppf_refine.hip fills its model levels), one workgroup
//   ossid_sym_score   one workgroup per candidate: every query is transformed in f64 (8.7's written order), rounded to f32
//                     and probed (cell_probe, worst = tol * tol); the workgroup reduces the misses, the largest accepted
//                     d2 (on its bits) and the integer sum of the quantised accepted d2
// Integer arithmetic past the probe, no float atomics, no random numbers: every result is independent of arrival order and
// bit-equal to tests/ref_symmetry.py, which searches the neighbours by brute force.
#include <float.h>
#include <math.h>

#include "cell_grid.h"
#include "workgroup.h"

namespace {

constexpr int MAX_CELLS = 32768;
constexpr int GNT = 1024;                    // grid build workgroup
constexpr int SNT = 256;                     // score workgroup

struct SymHeader {                           // at the start of the grid buffer, written by the grid kernel
    CellGrid g;
    int ncell, nt;
    float tol;                               // the tolerance the cells were sized for
};

// grid buffer: header | start int [MAX_CELLS + 1], cursor int [MAX_CELLS] | sorted float4 [Nt] (x, y, z, index as bits)
constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
constexpr size_t header_bytes() { return (sizeof(SymHeader) + 63) & ~(size_t)63; }
constexpr size_t table_bytes() { return align16((size_t)(2 * MAX_CELLS + 1) * 4); }
size_t grid_bytes(int Nt) { return header_bytes() + table_bytes() + (size_t)Nt * 16; }

bool tol_ok(float tol) { return tol > 0.0f && isfinite(tol) && tol * tol > 0.0f && isfinite(tol * tol); }

// one workgroup: the targets' box, the grid, the counting sort (the order inside a cell is free: the probe takes the
// lexicographic minimum of (d2, index))
__global__ __launch_bounds__(GNT) void sym_grid_kernel(const float* __restrict__ P, int Nt, float tol, void* __restrict__ grid) {
    __shared__ float red[GNT / 64][6];
    __shared__ int wsum[GNT / 64];
    __shared__ SymHeader sh;
    int* start = (int*)((char*)grid + header_bytes());
    int* cursor = start + MAX_CELLS + 1;
    float4* sorted = (float4*)((char*)grid + header_bytes() + table_bytes());
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = threadIdx.x; i < Nt; i += GNT) {
        const float x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
        mn[0] = fminf(mn[0], x), mn[1] = fminf(mn[1], y), mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x), mx[1] = fmaxf(mx[1], y), mx[2] = fmaxf(mx[2], z);
    }
    wg_bbox3<GNT / 64>(mn, mx, red);
    if (threadIdx.x == 0) {
        CellGrid g = cell_grid_size(mn, mx, tol, MAX_CELLS);
        // the one-cell grid: lo = 0, so that (x - lo) * 0 is 0 for every finite x (a box whose extent overflows f32
        // would make it inf * 0 for the queries at its far end). Also whatever a box without a finite point sizes to.
        const bool sane = g.n[0] >= 1 && g.n[1] >= 1 && g.n[2] >= 1 && (long long)g.n[0] * g.n[1] * g.n[2] <= MAX_CELLS;
        if (!sane || g.inv_h == 0.0f) {
            g.n[0] = g.n[1] = g.n[2] = 1, g.inv_h = 0.0f;
            g.lo[0] = g.lo[1] = g.lo[2] = 0.0f;
        }
        sh.g = g, sh.ncell = g.n[0] * g.n[1] * g.n[2], sh.nt = Nt, sh.tol = tol;
        *(SymHeader*)grid = sh;
    }
    __syncthreads();
    const CellGrid g = sh.g;
    const int ncell = sh.ncell;
    for (int c = threadIdx.x; c < ncell; c += GNT) cursor[c] = 0;
    __threadfence();
    __syncthreads();
    for (int i = threadIdx.x; i < Nt; i += GNT) atomicAdd(&cursor[cell_of(g, P[3 * i], P[3 * i + 1], P[3 * i + 2])], 1);
    __threadfence();
    __syncthreads();
    wg_scan_range<GNT / 64>(cursor, ncell, wsum, [&](int c, int base) { start[c] = base, cursor[c] = base; });
    if (threadIdx.x == 0) start[ncell] = Nt;
    __threadfence();
    __syncthreads();
    for (int i = threadIdx.x; i < Nt; i += GNT) {
        const float x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
        const int pos = atomicAdd(&cursor[cell_of(g, x, y, z)], 1);
        sorted[pos] = make_float4(x, y, z, __int_as_float(i));
    }
}

// the grid's storage for cell_probe: read through L2, which every workgroup shares. The positions are clamped to the Nt
// sorted points, so that whatever the cell table holds nothing outside the buffer is read.
struct SymCells {
    const int* start;
    const float4* srt;
    int nt;
    __device__ __forceinline__ void run(int first, int last, int& b, int& e) const {
        b = max(start[first], 0), e = min(start[last + 1], nt);
    }
    __device__ __forceinline__ float4 point(int p) const { return srt[p]; }
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (unsigned long long)__shfl_xor((long long)v, m);
    return v;
}

__global__ __launch_bounds__(SNT) void sym_score_kernel(const void* __restrict__ grid, int Nt, const float* __restrict__ Q, int Mq,
                                                        const double* __restrict__ T, float tol, int32_t* __restrict__ miss,
                                                        float* __restrict__ worst_d2, int64_t* __restrict__ sum_q) {
    __shared__ int s_miss[SNT / 64], s_max[SNT / 64];
    __shared__ unsigned long long s_sum[SNT / 64];
    const SymHeader hdr = *(const SymHeader*)grid;
    const int c = blockIdx.x;
    // a header that ossid_sym_grid did not write for these Nt targets and this tol is not followed: every query misses
    const bool built = hdr.nt == Nt && hdr.tol == tol && hdr.g.n[0] >= 1 && hdr.g.n[1] >= 1 && hdr.g.n[2] >= 1 &&
                       (long long)hdr.g.n[0] * hdr.g.n[1] * hdr.g.n[2] == hdr.ncell && hdr.ncell <= MAX_CELLS;
    const SymCells cells = {(const int*)((const char*)grid + header_bytes()),
                            (const float4*)((const char*)grid + header_bytes() + table_bytes()), Nt};
    const double* t = T + 16 * (size_t)c;
    double r[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) r[q] = t[q];
    const float worst = tol * tol;
    const double scale = (double)worst;
    int n_miss = 0, max_bits = 0;
    unsigned long long sum = 0;
    for (int i = threadIdx.x; i < Mq; i += SNT) {
        const double x = (double)Q[3 * i], y = (double)Q[3 * i + 1], z = (double)Q[3 * i + 2];
        const float px = (float)(((r[0] * x + r[1] * y) + r[2] * z) + r[3]);
        const float py = (float)(((r[4] * x + r[5] * y) + r[6] * z) + r[7]);
        const float pz = (float)(((r[8] * x + r[9] * y) + r[10] * z) + r[11]);
        CellHit h = {worst, INT_MAX, -1};
        if (built) h = cell_probe(hdr.g, cells, px, py, pz, worst);
        if (h.j == INT_MAX) {
            ++n_miss;
        } else {
            max_bits = max(max_bits, __float_as_int(h.d2));                  // d2 >= 0: the order of the bits is the floats'
            sum += (unsigned long long)(((double)h.d2 / scale) * 4294967296.0);
        }
    }
    n_miss = wave_sum_i32(n_miss), max_bits = wave_max_i32(max_bits), sum = wave_sum_u64(sum);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_miss[wv] = n_miss, s_max[wv] = max_bits, s_sum[wv] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < SNT / 64; ++w) n_miss += s_miss[w], max_bits = max(max_bits, s_max[w]), sum += s_sum[w];
    miss[c] = n_miss, worst_d2[c] = __int_as_float(max_bits), sum_q[c] = (int64_t)sum;
}

}  // namespace

size_t ossid_sym_grid_nbytes(int Nt) { return Nt >= 1 && Nt <= OSSID_SYM_MAX_TARGETS ? grid_bytes(Nt) : 0; }

int ossid_sym_grid(const float* targets, int Nt, float tol, void* grid, size_t grid_bytes_, void* stream) {
    const size_t need = ossid_sym_grid_nbytes(Nt);
    if (need == 0 || !tol_ok(tol) || !targets || !grid || grid_bytes_ < need || ((uintptr_t)grid & 15)) return OSSID_EINVAL;
    hipLaunchKernelGGL(sym_grid_kernel, dim3(1), dim3(GNT), 0, (hipStream_t)stream, targets, Nt, tol, grid);
    return ossid_launch_status();
}

int ossid_sym_score(const void* grid, size_t grid_bytes_, int Nt, const float* queries, int Mq, const double* transforms, int C,
                    float tol, int32_t* miss, float* worst_d2, int64_t* sum_q, void* stream) {
    const size_t need = ossid_sym_grid_nbytes(Nt);
    if (need == 0 || Mq < 1 || Mq > OSSID_SYM_MAX_QUERIES || C < 1 || C > OSSID_SYM_MAX_TRANSFORMS || !tol_ok(tol) || !grid ||
        grid_bytes_ < need || ((uintptr_t)grid & 15) || !queries || !transforms || !miss || !worst_d2 || !sum_q)
        return OSSID_EINVAL;
    hipLaunchKernelGGL(sym_score_kernel, dim3(C), dim3(SNT), 0, (hipStream_t)stream, grid, Nt, queries, Mq, transforms, tol, miss,
                       worst_d2, sum_q);
    return ossid_launch_status();
}
