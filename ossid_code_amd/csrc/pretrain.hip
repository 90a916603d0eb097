// The detector's pre-training batch straight from a rendered SceneBatch (SPEC.md section 15): one launch turns T chosen
// (scene, instance) targets into img / mask / bbox_gt / heatmap in the layouts DtoidNet.forward takes
// (models/dtoid/__init__.py:173-249), where the host route reads every image back and runs ossid_dtoid_prep_sample and
// ossid_mask_bbox_heatmap once per sample. HBM-bound and elementwise: ~7 MB per target at 480x640. A lane owns a run of 4
// pixels of the flattened frame -- three dwords of colour, one 16-byte instance load, a 16-byte store per plane -- when
// H*W is a multiple of 4 and the buffers are 16-byte aligned (every plane then starts aligned); any other frame takes
// the scalar path, one pixel per lane. The heat map (29x39 per target) rides in the same launch on a few extra workgroups.
// The box comes from gt_info's bbox_visib, so nothing is reduced here and nothing is read back.
#include "common.h"

namespace {

struct BatchArgs {
    const uint8_t* color;      // u8 [S][H][W][3]
    const int32_t* instance;   // int32 [S][H][W]
    const int32_t* gt_info;    // int32 [I][12]
    const int32_t* targets;    // int32 [T][2] = (s, i)
    const float* jitter;       // f32 [T][8] or null
    float* img;                // f32 [T][3][H][W]
    float* mask;               // f32 [T][1][H][W]
    float* bbox;               // f32 [T][5]
    double* heat;              // f64 [T][hh][hw]
    int S, I, T, n, hh, hw;    // n = H*W
    int px_blocks;             // workgroups of the pixel part per target; the heat map's follow
    double scale, sigma;
};

// 15.3's steps 2-8 on v = (float)u8 / 255.0f of channel c at flat pixel p; every operation rounds to f32 on its own
// (the library is built with -ffp-contract=off)
__device__ __forceinline__ float jitter_px(float v, float gain, float bias, float amp, uint32_t seed, uint32_t p, uint32_t c) {
    v = v * gain;
    v = v + bias;
    uint32_t k = seed + 0x9E3779B9u * (3u * p + c);
    k ^= k >> 16;
    k *= 0x7feb352du;
    k ^= k >> 15;
    k *= 0x846ca68bu;
    k ^= k >> 16;
    const float u = (float)(k >> 8) * 5.9604644775390625e-08f;     // 2^-24: exact
    const float d = u - 0.5f;
    v = v + d * amp;
    v = v > 0.0f ? v : 0.0f;                                       // NaN and -0 become +0
    return v < 1.0f ? v : 1.0f;
}

template <bool VEC>
__global__ __launch_bounds__(256) void scene_dtoid_batch_kernel(BatchArgs a) {
    for (int t = blockIdx.y; t < a.T; t += gridDim.y) {
        const int s = a.targets[2 * t], i = a.targets[2 * t + 1];
        const bool ok = s >= 0 && s < a.S && i >= 0 && i < a.I;    // a bad row writes zeros and the empty box, reads nothing
        if ((int)blockIdx.x >= a.px_blocks) {
            // ---- heat map around the box centre (14.2's formula), and the box row itself -------------------------------
            int bx = -1, by = -1, bw = -1, bh = -1;
            if (ok) bx = a.gt_info[12 * i + 7], by = a.gt_info[12 * i + 8], bw = a.gt_info[12 * i + 9], bh = a.gt_info[12 * i + 10];
            const bool full = bx >= 0 && by >= 0 && bw > 0 && bh > 0;
            const int x1 = full ? bx : 1 << 30, y1 = full ? by : 1 << 30, x2 = full ? bx + bw - 1 : -1, y2 = full ? by + bh - 1 : -1;
            const int k = ((int)blockIdx.x - a.px_blocks) * 256 + (int)threadIdx.x;
            if (k == 0) {
                float* b = a.bbox + 5 * (size_t)t;
                b[0] = (float)x1, b[1] = (float)y1, b[2] = (float)x2, b[3] = (float)y2, b[4] = full ? 1.0f : -1.0f;
            }
            if (k < a.hh * a.hw) {
                const int y = k / a.hw, x = k - y * a.hw;
                const double cx = ((double)x1 + (double)x2) / 2.0 * a.scale, cy = ((double)y1 + (double)y2) / 2.0 * a.scale;
                const double dx = (double)x - cx, dy = (double)y - cy;
                const double dst = sqrt(dx * dx + dy * dy);
                a.heat[(size_t)t * a.hh * a.hw + k] = full ? exp(-(dst * dst / (2.0 * a.sigma * a.sigma))) : 0.0;
            }
            continue;
        }
        // ---- image and mask planes -------------------------------------------------------------------------------------
        const size_t n = (size_t)a.n;
        float* img = a.img + (size_t)t * 3 * n;
        float* mask = a.mask + (size_t)t * n;
        float g[3] = {1.0f, 1.0f, 1.0f}, b[3] = {0.0f, 0.0f, 0.0f}, amp = 0.0f;
        uint32_t seed = 0;
        const bool jit = a.jitter != nullptr;
        if (jit) {
            const float* j = a.jitter + 8 * (size_t)t;
            g[0] = j[0], g[1] = j[1], g[2] = j[2], b[0] = j[3], b[1] = j[4], b[2] = j[5], amp = j[6];
            seed = __float_as_uint(j[7]);
        }
        if (VEC) {
            const int q = blockIdx.x * 256 + threadIdx.x;          // pixels 4q .. 4q+3 of the flattened frame
            if (q >= a.n / 4) continue;
            const size_t p0 = 4 * (size_t)q;
            float v[3][4];
            float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ok) {
                const uint32_t* c32 = (const uint32_t*)(a.color + ((size_t)s * n + p0) * 3);
                const uint32_t w0 = c32[0], w1 = c32[1], w2 = c32[2];      // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
                const int4 id = *(const int4*)(a.instance + (size_t)s * n + p0);
                v[0][0] = (float)(w0 & 255u), v[1][0] = (float)((w0 >> 8) & 255u), v[2][0] = (float)((w0 >> 16) & 255u);
                v[0][1] = (float)(w0 >> 24), v[1][1] = (float)(w1 & 255u), v[2][1] = (float)((w1 >> 8) & 255u);
                v[0][2] = (float)((w1 >> 16) & 255u), v[1][2] = (float)(w1 >> 24), v[2][2] = (float)(w2 & 255u);
                v[0][3] = (float)((w2 >> 8) & 255u), v[1][3] = (float)((w2 >> 16) & 255u), v[2][3] = (float)(w2 >> 24);
                m = make_float4(id.x == i ? 1.0f : 0.0f, id.y == i ? 1.0f : 0.0f, id.z == i ? 1.0f : 0.0f, id.w == i ? 1.0f : 0.0f);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = 0.0f;
                    if (ok) {
                        o[e] = v[c][e] / 255.0f;
                        if (jit) o[e] = jitter_px(o[e], g[c], b[c], amp, seed, (uint32_t)p0 + e, c);
                    }
                }
                *(float4*)(img + c * n + p0) = make_float4(o[0], o[1], o[2], o[3]);
            }
            *(float4*)(mask + p0) = m;
        } else {
            const int p = blockIdx.x * 256 + threadIdx.x;
            if (p >= a.n) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float o = 0.0f;
                if (ok) {
                    o = (float)a.color[((size_t)s * n + p) * 3 + c] / 255.0f;
                    if (jit) o = jitter_px(o, g[c], b[c], amp, seed, (uint32_t)p, c);
                }
                img[c * n + p] = o;
            }
            mask[p] = ok && a.instance[(size_t)s * n + p] == i ? 1.0f : 0.0f;
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int ossid_scene_dtoid_batch(const uint8_t* color, const int32_t* instance, const int32_t* gt_info, int S, int H, int W,
                                       int I, const int32_t* targets, int T, const float* jitter, int heat_h, int heat_w,
                                       double sigma, float* img_out, float* mask_out, float* bbox_out, double* heatmap_out,
                                       void* stream) {
    if (!color || !instance || !gt_info || !targets || !img_out || !mask_out || !bbox_out || !heatmap_out) return OSSID_EINVAL;
    if (S <= 0 || H <= 0 || W <= 0 || I <= 0 || T < 1 || heat_h <= 0 || heat_w <= 0) return OSSID_EINVAL;
    if ((long long)H * W >= (1LL << 30) || (long long)heat_h * heat_w >= (1LL << 30) || !(sigma > 0.0)) return OSSID_EINVAL;
    BatchArgs a;
    a.color = color, a.instance = instance, a.gt_info = gt_info, a.targets = targets, a.jitter = jitter;
    a.img = img_out, a.mask = mask_out, a.bbox = bbox_out, a.heat = heatmap_out;
    a.S = S, a.I = I, a.T = T, a.n = H * W, a.hh = heat_h, a.hw = heat_w;
    a.scale = (double)heat_h / (double)H, a.sigma = sigma;
    const bool vec = a.n % 4 == 0 && aligned16(color) && aligned16(instance) && aligned16(img_out) && aligned16(mask_out);
    a.px_blocks = ((vec ? a.n / 4 : a.n) + 255) / 256;
    const dim3 grid(a.px_blocks + (heat_h * heat_w + 255) / 256, T < 65535 ? T : 65535);
    if (vec)
        hipLaunchKernelGGL(scene_dtoid_batch_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(scene_dtoid_batch_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return ossid_launch_status();
}
