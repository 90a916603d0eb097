// Cluttered multi-object RGB-D scenes with ground truth (SPEC.md section 13): many instances of the meshes of an atlas in
// one frame per scene, with mutual occlusion, per-pixel instance labels, amodal masks, the numbers of BOP's
// scene_gt_info.json and the depth corruption the reference applies to its pre-training renders
// (utils/augmentation.py:5-26, over the BlenderProc scenes of datasets/render_dataset.py:81-189). The arithmetic of a
// sample, the triangle fetch, the wave walk over large boxes and the winner's setup are raster_common.h's, the ones
// csrc/raster.hip runs, so a scene image is, per pixel, the winner by (bits(z), instance) among
// what ossid_raster_color renders for each instance alone, bit for bit.
//
// ossid_scene_render, three launches on the caller's stream, nothing read back:
//   prepare   one thread per (instance, vertex) record -- the instances' records lie back to back in the workspace at the
//             offsets the caller computed -- and the clears: visibility keys to KFAR, amodal masks to 0;
//   triangles a flattened work list over (instance, triangle group): one wave per item, the instance found by a binary
//             search of the caller's prefix sums, so a 12-face box and a 300 000-face scan both fill waves. A mesh of nf
//             faces is cut into groups of tpw = clamp(ceil(nf / 64), 1, 64) triangles; meshes of at most 64 faces (tables,
//             boxes: few, large triangles) get one triangle per group and SPLIT items per group that share its large box by
//             rows of tiles. Small boxes are walked by their lane, large ones by the whole wave, 8 x 8 samples per step
//             (wave_walk). Every covered sample sets its bit in the instance's amodal mask BEFORE the depth test (the
//             wave walk ORs one byte per tile row, not one bit per sample) and then competes for the pixel's key
//             bits(z) << 32 | local instance << 22 | face by atomicMin behind a plain load;
//   resolve   one thread per (scene, pixel): the winner's colour, depth, global instance, face and facing, or the background.
// Minima and ORs do not depend on the order of arrival: every output is bit-reproducible whatever the schedule.
//
// ossid_scene_render_textured is the same three launches with an ossid_scene_tex behind the descriptor: a per-mesh
// texture table (first texel of the mesh's mip chain, Ht, Wt; Ht = 0: vertex colours), the atlas's UV rows and the chains
// back to back. The kernels are templates over a pack `Tex...` that is empty for ossid_scene_render -- whose
// instantiations therefore hold no texture code and take the arguments they always took -- and one ossid_scene_tex for
// the textured entry. There load_instance also checks the mesh's row of the table against mip_texels, so an instance
// whose row leads outside the chains is not drawn by any of the three, and the resolve colours a winner whose mesh has
// Ht > 0 by raster_common.h's sample_texture, the function csrc/raster.hip's textured resolve calls.
//
// ossid_scene_gt_info: one thread per (instance, 32-pixel mask word); popcounts, per-wave shuffles, a per-workgroup LDS
// step, then one integer atomic per counter per workgroup. ossid_scene_sensor: one thread per pixel, no random numbers.
#include <cmath>

#include "raster_common.h"

namespace {

constexpr int SPLIT = 8;             // work items per group of a mesh of at most 64 faces
constexpr int LOCAL_BITS = 10, FACE_BITS = 22;
static_assert((1 << LOCAL_BITS) == OSSID_SCENE_MAX_INSTANCES && (1 << FACE_BITS) == OSSID_RASTER_MAX_FACES, "key layout");
constexpr int MAX_TOTAL = 1 << 29;   // atlas vertices / faces: 3 * index stays inside int32

__host__ __device__ inline int tris_per_group(int nf) {
    const int t = (nf + 63) / 64;
    return t < 1 ? 1 : (t > 64 ? 64 : t);
}

__host__ __device__ inline int items_of(int nf) {
    if (nf <= 0) return 0;
    const int tpw = tris_per_group(nf), groups = (nf + tpw - 1) / tpw;
    return tpw == 1 ? groups * SPLIT : groups;
}

// Largest j in [0, n) with first[j * stride] <= v, for a non-decreasing table with first[0] <= v.
__device__ __forceinline__ int owner(const int32_t* __restrict__ first, int n, int stride, int v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[(size_t)mid * stride] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// What a wave needs of one instance; ok = every index it leads to lies inside its array.
struct Inst {
    int scene, local, v0, nv, f0, nf, rec0;
    bool ok;
};

// The texture table's row of mesh m leads to texels inside [0, mip_texels) only (a vertex-coloured row, Ht = 0, leads
// to none); without a table every mesh is vertex-coloured.
__device__ __forceinline__ bool tex_row_ok(int) { return true; }
__device__ __forceinline__ bool tex_row_ok(int m, const ossid_scene_tex& t) {
    const int64_t t0 = t.tex_table[3 * (size_t)m], Ht = t.tex_table[3 * (size_t)m + 1], Wt = t.tex_table[3 * (size_t)m + 2];
    if (Ht <= 0) return Ht == 0;
    return Ht <= OSSID_TEXTURE_MAX_SIDE && Wt >= 1 && Wt <= OSSID_TEXTURE_MAX_SIDE && t0 >= 0 && t0 <= t.mip_texels &&
           (int64_t)tex_total_texels((int)Ht, (int)Wt) <= t.mip_texels - t0;
}

template <typename... Tex>
__device__ __forceinline__ Inst load_instance(const ossid_scene_desc& d, int inst, const Tex&... tex) {
    Inst r = {};
    const int m = d.instance_mesh[inst];
    if (m < 0 || m >= d.K || !tex_row_ok(m, tex...)) return r;
    r.v0 = d.meshes[4 * m], r.nv = d.meshes[4 * m + 1], r.f0 = d.meshes[4 * m + 2], r.nf = d.meshes[4 * m + 3];
    r.rec0 = d.offsets[2 * (size_t)inst + 1];
    r.scene = owner(d.scene_first, d.S, 1, inst);
    r.local = inst - d.scene_first[r.scene];
    r.ok = r.v0 >= 0 && r.nv >= 0 && r.nv <= d.Vt - r.v0 && r.f0 >= 0 && r.nf >= 0 && r.nf <= OSSID_RASTER_MAX_FACES &&
           r.nf <= d.Ft - r.f0 && r.rec0 >= 0 && r.nv <= d.records - r.rec0 && r.local >= 0 &&
           r.local < OSSID_SCENE_MAX_INSTANCES;
    return r;
}

template <typename... Tex>
__global__ __launch_bounds__(256) void scene_prepare_kernel(ossid_scene_desc d, VRec* __restrict__ rec,
                                                            unsigned long long* __restrict__ keys, Tex... tex) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    const size_t npix = (size_t)d.S * d.H * d.W, nwords = (size_t)d.I * d.H * ((d.W + 31) / 32);
    for (size_t i = tid; i < npix; i += nthreads) keys[i] = KFAR;
    for (size_t i = tid; i < nwords; i += nthreads) d.amodal_out[i] = 0u;
    const int lane = threadIdx.x & 63;
    for (size_t i = tid; i < (size_t)d.records; i += nthreads) {
        // the wave's 64 records mostly belong to one instance: one search for the wave, then a short walk per lane
        int inst = owner(d.offsets + 1, d.I, 2, __builtin_amdgcn_readfirstlane((int)i - lane));
        while (inst + 1 < d.I && d.offsets[2 * (size_t)(inst + 1) + 1] <= (int)i) ++inst;
        const Inst in = load_instance(d, inst, tex...);
        const int k = (int)i - in.rec0;
        VRec r;
        r.sx = INT_MIN, r.sy = 0, r.rz = 0.0;
        if (in.ok && k >= 0 && k < in.nv) {
            const float* c = d.cams + 4 * (size_t)in.scene;
            r = project_vertex(d.vertices, in.v0 + k, d.transforms + 16 * (size_t)inst, c[0], c[1], c[2], c[3], d.z_near);
        }
        rec[i] = r;
    }
}

__device__ __forceinline__ void or_bits(unsigned* p, unsigned bits) {
    // bits are only ever set: a stale load costs a useless atomic, and a closed mesh covers most samples twice
    if ((__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(p, bits);
}

template <typename... Tex>
__global__ __launch_bounds__(256) void scene_tri_kernel(ossid_scene_desc d, const VRec* __restrict__ rec,
                                                        unsigned long long* __restrict__ keys, int o, Tex... tex) {
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (item >= d.work_items) return;                      // whole waves leave: nothing below synchronises the workgroup
    const int inst = owner(d.offsets, d.I, 2, item);
    const Inst in = load_instance(d, inst, tex...);
    if (!in.ok) return;
    const int g = item - d.offsets[2 * (size_t)inst];
    if (g < 0 || g >= items_of(in.nf)) return;
    const int tpw = tris_per_group(in.nf), split = tpw == 1 ? SPLIT : 1;
    const int part = g % split, tri = (g / split) * tpw + lane;
    const int Wd = (d.W + 31) / 32;
    const VRec* vr = rec + in.rec0;
    unsigned long long* zb = keys + (size_t)in.scene * d.H * d.W;
    unsigned* am = d.amodal_out + (size_t)inst * d.H * Wd;
    const unsigned low = (unsigned)in.local << FACE_BITS;
    Tri t = {};
    long long A = 0;
    const TriKind kind = lane < tpw && tri < in.nf ? fetch_triangle(d.faces + 3 * (size_t)(in.f0 + tri), in.nv, vr, o, d.H, d.W, t, A)
                                                   : TRI_EMPTY;
    if (kind == TRI_SMALL && part == 0)
        for (int y = t.ya; y <= t.yb; ++y)
            for (int x = t.xa; x <= t.xb; ++x)
                if (shade(t, (double)A, x, y, o, d.W, zb, low | (unsigned)tri))
                    or_bits(am + (size_t)y * Wd + (x >> 5), 1u << (x & 31));
    // the items of a split group take every split-th row of tiles
    const int lx = lane & 7, ly = lane >> 3;
    wave_walk(t, A, kind == TRI_LARGE, part, split, [&](const Tri& s, double area, int src, int x0, int x, int y, bool in_box) {
        const bool cov = in_box && shade(s, area, x, y, o, d.W, zb, low | (unsigned)(tri - lane + src));
        // the tile row's 8 coverage bits in one OR by its first lane (two when the row straddles a mask word)
        const unsigned row = (unsigned)(__ballot(cov) >> (8 * ly)) & 0xffu;
        if (lx == 0 && row) {
            unsigned* p = am + (size_t)y * Wd + (x0 >> 5);
            const int sh = x0 & 31;
            or_bits(p, row << sh);
            if (sh > 24 && (row >> (32 - sh))) or_bits(p + 1, row >> (32 - sh));
        }
    });
}

// The surface of a winner of a textured atlas (mesh m, vertices from v0, face i0 i1 i2) at pixel (x, y): the mesh's
// texture when its row of the table has Ht > 0, its vertex colours otherwise. Returns the level fetched, -1 for colours.
__device__ __forceinline__ int shade_winner(const ossid_scene_desc& d, const ossid_scene_tex& t, const VRec* __restrict__ vr,
                                            int m, int v0, int i0, int i1, int i2, int x, int y, int o, int c[3]) {
    // the row passed tex_row_ok when the winner's key was written: the chain lies inside the buffer
    const int Ht = (int)t.tex_table[3 * (size_t)m + 1];
    if (Ht <= 0) {
        sample_color(vr, d.colors + 3 * (size_t)v0, i0, i1, i2, x, y, o, c);
        return -1;
    }
    return sample_texture(vr, i0, i1, i2, t.uvs + 2 * (size_t)v0, (const unsigned*)t.mips + t.tex_table[3 * (size_t)m], Ht,
                          (int)t.tex_table[3 * (size_t)m + 2], x, y, o, c);
}
__device__ __forceinline__ void store_lod(size_t, int) {}
__device__ __forceinline__ void store_lod(size_t i, int lod, const ossid_scene_tex& t) {
    if (t.lod_out) t.lod_out[i] = lod;
}

// SPEC 13.4, one thread per (scene, pixel). TEX says whether the pack holds the textured entry's ossid_scene_tex.
template <bool TEX, typename... Tex>
__global__ __launch_bounds__(256) void scene_resolve_kernel(ossid_scene_desc d, const VRec* __restrict__ rec,
                                                            const unsigned long long* __restrict__ keys, int o, Tex... tex) {
    static_assert(sizeof...(Tex) == (TEX ? 1 : 0), "one ossid_scene_tex, or none");
    const size_t hw = (size_t)d.H * d.W, npix = (size_t)d.S * hw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        const int scene = (int)(i / hw);
        const int pix = (int)(i - (size_t)scene * hw), y = pix / d.W, x = pix - y * d.W;
        float z = 0.0f, facing = 0.0f;
        int face = -1, inst = -1, lod = -1, c[3] = {0, 0, 0};
        if (key != KFAR) {
            // written by a usable triangle of a checked instance: every index below lies inside its array
            face = (int)((unsigned)key & ((1u << FACE_BITS) - 1u));
            inst = d.scene_first[scene] + (int)(((unsigned)key >> FACE_BITS) & ((1u << LOCAL_BITS) - 1u));
            z = __uint_as_float((unsigned)(key >> 32));
            const int m = d.instance_mesh[inst], v0 = d.meshes[4 * m], f0 = d.meshes[4 * m + 2];
            const int32_t* f = d.faces + 3 * (size_t)(f0 + face);
            const int i0 = f[0], i1 = f[1], i2 = f[2];
            // the untextured instantiation keeps the call it always made: its code is the one it always was
            if constexpr (TEX)
                lod = shade_winner(d, tex..., rec + d.offsets[2 * (size_t)inst + 1], m, v0, i0, i1, i2, x, y, o, c);
            else
                sample_color(rec + d.offsets[2 * (size_t)inst + 1], d.colors + 3 * (size_t)v0, i0, i1, i2, x, y, o, c);
            if (d.facing_out) {
                const float* T = d.transforms + 16 * (size_t)inst;
                float X0, Y0, Z0, X1, Y1, Z1, X2, Y2, Z2;
                camera_point(d.vertices, v0 + i0, T, X0, Y0, Z0);
                camera_point(d.vertices, v0 + i1, T, X1, Y1, Z1);
                camera_point(d.vertices, v0 + i2, T, X2, Y2, Z2);
                const double ax = (double)X1 - (double)X0, ay = (double)Y1 - (double)Y0, az = (double)Z1 - (double)Z0;
                const double bx = (double)X2 - (double)X0, by = (double)Y2 - (double)Y0, bz = (double)Z2 - (double)Z0;
                const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
                const double nn = (nx * nx + ny * ny) + nz * nz;
                facing = nn == 0.0 ? 0.0f : (float)(fabs(nz) / sqrt(nn));
            }
        } else if (d.background) {
            const unsigned char* bg = d.background + 3 * ((d.Sb == 1 ? 0 : (size_t)scene * hw) + pix);
            c[0] = bg[0], c[1] = bg[1], c[2] = bg[2];
        }
        d.depth_out[i] = z;
        d.instance_out[i] = inst;
        d.color_out[3 * i] = (unsigned char)c[0], d.color_out[3 * i + 1] = (unsigned char)c[1];
        d.color_out[3 * i + 2] = (unsigned char)c[2];
        if (d.face_out) d.face_out[i] = face;
        if (d.facing_out) d.facing_out[i] = facing;
        store_lod(i, lod, tex...);
    }
}

// ---- gt-info (SPEC 13.5) -------------------------------------------------------------------------------------------------------
// Slots of an instance's row while it accumulates: 0-2 the counts, 3-6 the amodal box and 7-10 the visible box as
// (min x, min y, max x, max y), 11 spare; the finish kernel turns the boxes into (x, y, w, h).
constexpr int GT = 12;

__global__ __launch_bounds__(256) void scene_gt_init_kernel(int32_t* __restrict__ out, int I) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)I * GT) return;
    const int k = (int)(i % GT);
    out[i] = (k == 3 || k == 4 || k == 7 || k == 8) ? INT_MAX : ((k == 5 || k == 6 || k == 9 || k == 10) ? -1 : 0);
}

__global__ __launch_bounds__(256) void scene_gt_count_kernel(const unsigned* __restrict__ amodal,
                                                             const int32_t* __restrict__ instance_img,
                                                             const float* __restrict__ sensor,
                                                             const int32_t* __restrict__ scene_first, int S, int H, int W,
                                                             int blocks_per_instance, int32_t* __restrict__ out) {
    const int inst = blockIdx.x / blocks_per_instance, blk = blockIdx.x - inst * blocks_per_instance;
    const int Wd = (W + 31) / 32, nwords = H * Wd, wi = blk * 256 + threadIdx.x;
    int v[11] = {0, 0, 0, INT_MAX, INT_MAX, -1, -1, INT_MAX, INT_MAX, -1, -1};
    if (wi < nwords) {
        unsigned word = amodal[(size_t)inst * nwords + wi];
        if (word) {
            const int y = wi / Wd, xw = 32 * (wi - y * Wd);
            const size_t row = ((size_t)owner(scene_first, S, 1, inst) * H + y) * W;
            v[0] = __popc(word);
            v[3] = xw + __ffs((int)word) - 1, v[5] = xw + 31 - __clz((int)word), v[4] = v[6] = y;
            while (word) {
                const int x = xw + __ffs((int)word) - 1;
                word &= word - 1;
                if (x >= W) break;                          // bits past the row's end are never set; never read past it
                v[2] += sensor[row + x] > 0.0f;
                if (instance_img[row + x] == inst) {
                    ++v[1];
                    v[7] = min(v[7], x), v[9] = max(v[9], x), v[8] = v[10] = y;
                }
            }
        }
    }
    __shared__ int part[4][11];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const int r = k < 3 ? wave_sum_i32(v[k]) : ((k == 3 || k == 4 || k == 7 || k == 8) ? wave_min_i32(v[k]) : wave_max_i32(v[k]));
        if (lane == 0) part[wv][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < 11) {
        const int k = threadIdx.x;
        const bool is_min = k == 3 || k == 4 || k == 7 || k == 8;
        int r = part[0][k];
        for (int w = 1; w < 4; ++w) r = k < 3 ? r + part[w][k] : (is_min ? min(r, part[w][k]) : max(r, part[w][k]));
        int32_t* p = out + (size_t)inst * GT + k;           // integers only: independent of the order of arrival
        if (k < 3) {
            if (r) atomicAdd(p, r);
        } else if (is_min) {
            if (r != INT_MAX) atomicMin(p, r);
        } else if (r >= 0) {
            atomicMax(p, r);
        }
    }
}

__global__ __launch_bounds__(256) void scene_gt_finish_kernel(int32_t* __restrict__ out, int I) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)I * 2) return;
    int32_t* b = out + (i / 2) * GT + 3 + 4 * (i % 2);
    if (b[2] < 0) {
        b[0] = b[1] = b[2] = b[3] = -1;
    } else {
        b[2] = b[2] - b[0] + 1, b[3] = b[3] - b[1] + 1;
    }
}

// ---- sensor (SPEC 13.6) ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scene_sensor_kernel(const float* __restrict__ depth, const float* __restrict__ facing,
                                                           int S, int H, int W, const float* __restrict__ thresholds,
                                                           const int32_t* __restrict__ n_rects,
                                                           const int32_t* __restrict__ rects, double units, double unit_inv,
                                                           uint16_t* __restrict__ depth_u16, float* __restrict__ depth_out,
                                                           unsigned char* __restrict__ keep_out) {
    const size_t hw = (size_t)H * W, npix = (size_t)S * hw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const int s = (int)(i / hw);
        const int pix = (int)(i - (size_t)s * hw), y = pix / W, x = pix - y * W;
        bool keep = facing[i] >= thresholds[s];
        const int n = min(max(n_rects[s], 0), OSSID_SCENE_MAX_RECTS);
        for (int k = 0; k < n; ++k) {
            const int32_t* r = rects + 4 * ((size_t)s * OSSID_SCENE_MAX_RECTS + k);
            if (y >= r[0] && y < r[1] && x >= r[2] && x < r[3]) keep = false;
        }
        double q = keep ? rint((double)depth[i] * units) : 0.0;
        if (!(q >= 0.0 && q <= 65535.0)) q = 0.0;           // what a 16-bit PNG cannot hold is an invalid pixel
        depth_u16[i] = (uint16_t)q;
        depth_out[i] = (float)(q * unit_inv);
        if (keep_out) keep_out[i] = keep;
    }
}

bool frame_ok(int S, int H, int W) {
    return S >= 1 && S <= OSSID_SCENE_MAX_SCENES && H > 0 && W > 0 && (long long)H * W <= OSSID_RASTER_MAX_PIXELS;
}

// Both render entries: the refusals, the workspace cut into records and keys, and the three launches, whose kernels take
// the pack after their own arguments.
template <typename... Tex>
int scene_render(const ossid_scene_desc* desc_host, void* workspace, size_t workspace_bytes, void* stream, Tex... tex) {
    if (!desc_host) return OSSID_EINVAL;
    const ossid_scene_desc d = *desc_host;
    const size_t need = ossid_scene_workspace_bytes(d.records, d.S, d.H, d.W);
    if (need == 0 || !workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) return OSSID_EINVAL;
    if (d.K < 1 || d.Vt < 1 || d.Vt > MAX_TOTAL || d.Ft < 0 || d.Ft > MAX_TOTAL || d.I < 0 ||
        (long long)d.I > (long long)d.S * OSSID_SCENE_MAX_INSTANCES || d.work_items < 0 || d.work_items > (1 << 30) ||
        !raster_frame_ok(d.H, d.W, d.pixel_offset, d.z_near))
        return OSSID_EINVAL;
    if (!d.vertices || !d.colors || (d.Ft > 0 && !d.faces) || !d.meshes || !d.scene_first || !d.cams || !d.offsets ||
        (d.I > 0 && (!d.instance_mesh || !d.transforms || !d.amodal_out)) || !d.color_out || !d.depth_out || !d.instance_out ||
        (d.background && d.Sb != 1 && d.Sb != d.S))
        return OSSID_EINVAL;
    const int o = snap_offset(d.pixel_offset);
    const size_t npix = (size_t)d.S * d.H * d.W, nwords = (size_t)d.I * d.H * ((d.W + 31) / 32);
    hipStream_t s = (hipStream_t)stream;
    VRec* rec = (VRec*)workspace;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + (size_t)d.records * sizeof(VRec));
    size_t work = npix > nwords ? npix : nwords;
    if ((size_t)d.records > work) work = (size_t)d.records;
    hipLaunchKernelGGL(scene_prepare_kernel<Tex...>, dim3(grid_for(work)), dim3(256), 0, s, d, rec, keys, tex...);
    if (d.work_items > 0 && d.I > 0)
        hipLaunchKernelGGL(scene_tri_kernel<Tex...>, dim3((unsigned)((d.work_items + 3) / 4)), dim3(256), 0, s, d, rec, keys, o,
                           tex...);
    hipLaunchKernelGGL((scene_resolve_kernel<sizeof...(Tex) != 0, Tex...>), dim3(grid_for(npix)), dim3(256), 0, s, d, rec, keys,
                       o, tex...);
    return ossid_launch_status();
}

}  // namespace

extern "C" {

int ossid_scene_work_items(int n_faces) {
    return n_faces < 0 || n_faces > OSSID_RASTER_MAX_FACES ? -1 : items_of(n_faces);
}

size_t ossid_scene_workspace_bytes(int records, int S, int H, int W) {
    if (records < 0 || !frame_ok(S, H, W)) return 0;
    return (size_t)records * sizeof(VRec) + (size_t)S * H * W * sizeof(unsigned long long);
}

int ossid_scene_render(const ossid_scene_desc* desc_host, void* workspace, size_t workspace_bytes, void* stream) {
    return scene_render(desc_host, workspace, workspace_bytes, stream);
}

int ossid_scene_render_textured(const ossid_scene_desc* desc_host, const ossid_scene_tex* tex_host, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (!tex_host || !tex_host->uvs || !tex_host->mips || !tex_host->tex_table || ((uintptr_t)tex_host->mips & 3) != 0 ||
        tex_host->mip_texels < 1)
        return OSSID_EINVAL;
    return scene_render(desc_host, workspace, workspace_bytes, stream, *tex_host);
}

int ossid_scene_gt_info(const uint32_t* amodal, const int32_t* instance_img, const float* sensor_depth,
                        const int32_t* scene_first, int I, int S, int H, int W, int32_t* gt_info, void* stream) {
    if (I < 0 || !frame_ok(S, H, W) || (long long)I > (long long)S * OSSID_SCENE_MAX_INSTANCES || !instance_img ||
        !sensor_depth || !scene_first || (I > 0 && (!amodal || !gt_info)))
        return OSSID_EINVAL;
    if (I == 0) return OSSID_OK;
    const int bpi = (H * ((W + 31) / 32) + 255) / 256;
    if ((long long)I * bpi > INT_MAX) return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(scene_gt_init_kernel, dim3((I * GT + 255) / 256), dim3(256), 0, s, gt_info, I);
    hipLaunchKernelGGL(scene_gt_count_kernel, dim3((unsigned)(I * bpi)), dim3(256), 0, s, amodal, instance_img, sensor_depth,
                       scene_first, S, H, W, bpi, gt_info);
    hipLaunchKernelGGL(scene_gt_finish_kernel, dim3((I * 2 + 255) / 256), dim3(256), 0, s, gt_info, I);
    return ossid_launch_status();
}

int ossid_scene_sensor(const float* depth, const float* facing, int S, int H, int W, const float* thresholds,
                       const int32_t* n_rects, const int32_t* rects, double units, double unit_inv, uint16_t* depth_u16,
                       float* depth_out, uint8_t* keep, void* stream) {
    if (!depth || !facing || !frame_ok(S, H, W) || !thresholds || !n_rects || !rects || !(units > 0.0) || !std::isfinite(units) ||
        !(unit_inv > 0.0) || !std::isfinite(unit_inv) || !depth_u16 || !depth_out)
        return OSSID_EINVAL;
    hipLaunchKernelGGL(scene_sensor_kernel, dim3(grid_for((size_t)S * H * W)), dim3(256), 0, (hipStream_t)stream, depth, facing,
                       S, H, W, thresholds, n_rects, rects, units, unit_inv, depth_u16, depth_out, keep);
    return ossid_launch_status();
}

}  // extern "C"
