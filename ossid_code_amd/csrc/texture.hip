// The mip chain of a UV texture (SPEC.md 7.15): level 0 is the image, every further level the rounded 2 x 2 box of the
// level before it, integers only, so that the chain is bit-reproducible and equal to the numpy restatement
// tests/ref_raster_textured.py. One launch per level on the caller's stream (at most 14: a side is at most 8192), nothing
// allocated or read back. The layout of the buffer and the sampler that reads it are in texture.h.
#include "texture.h"

namespace {

// level 0: u8 [Ht][Wt][3] -> one 32-bit texel R | G << 8 | B << 16, the pad byte 0
__global__ __launch_bounds__(256) void texture_pack_kernel(const unsigned char* __restrict__ image, size_t n,
                                                           unsigned* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned char* p = image + 3 * i;
        out[i] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    }
}

// level l + 1 from level l (h x w): per channel (a + b + c + d + 2) div 4 over rows 2y, 2y + 1 and columns 2x, 2x + 1,
// the odd ones clamped to the last row / column
__global__ __launch_bounds__(256) void texture_down_kernel(const unsigned* __restrict__ src, int h, int w,
                                                           unsigned* __restrict__ dst) {
    const int h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
    const size_t n = (size_t)h2 * w2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / w2), x = (int)(i - (size_t)y * w2);
        const int y0 = 2 * y, y1 = min(2 * y + 1, h - 1), x0 = 2 * x, x1 = min(2 * x + 1, w - 1);
        const unsigned a = src[(size_t)y0 * w + x0], b = src[(size_t)y0 * w + x1], c = src[(size_t)y1 * w + x0],
                       d = src[(size_t)y1 * w + x1];
        unsigned o = 0u;
#pragma unroll
        for (int sh = 0; sh < 24; sh += 8)
            o |= (((((a >> sh) & 255u) + ((b >> sh) & 255u)) + (((c >> sh) & 255u) + ((d >> sh) & 255u)) + 2u) >> 2) << sh;
        dst[i] = o;
    }
}

}  // namespace

extern "C" {

size_t ossid_texture_mip_bytes(int Ht, int Wt) {
    if (Ht < 1 || Ht > OSSID_TEXTURE_MAX_SIDE || Wt < 1 || Wt > OSSID_TEXTURE_MAX_SIDE) return 0;
    return 4 * tex_total_texels(Ht, Wt);
}

int ossid_texture_levels(int Ht, int Wt) {
    if (Ht < 1 || Ht > OSSID_TEXTURE_MAX_SIDE || Wt < 1 || Wt > OSSID_TEXTURE_MAX_SIDE) return 0;
    return tex_top_level(Ht, Wt) + 1;
}

int ossid_texture_mips(const uint8_t* image, int Ht, int Wt, void* mips, size_t mip_bytes, void* stream) {
    const size_t need = ossid_texture_mip_bytes(Ht, Wt);
    if (need == 0 || !image || !mips || mip_bytes < need || ((uintptr_t)mips & 3) != 0) return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    unsigned* lv = (unsigned*)mips;
    int h = Ht, w = Wt;
    hipLaunchKernelGGL(texture_pack_kernel, dim3(grid_for((size_t)h * w)), dim3(256), 0, s, image, (size_t)h * w, lv);
    while (h > 1 || w > 1) {
        unsigned* next = lv + (size_t)h * w;
        const int h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
        hipLaunchKernelGGL(texture_down_kernel, dim3(grid_for((size_t)h2 * w2)), dim3(256), 0, s, lv, h, w, next);
        lv = next, h = h2, w = w2;
    }
    return ossid_launch_status();
}

}  // extern "C"
