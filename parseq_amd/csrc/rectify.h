// Rectification of quadrilateral text regions on the device: what a caller with a text detector does first.  Every
// region (image index, output size, eight coefficients) reads ONE of the call's shared source images through Pillow's PERSPECTIVE map and
// its bicubic filter, byte for byte Image.transform((w, h), Image.PERSPECTIVE, coef, Image.BICUBIC) with fill 0 (restated in
// tests/rectify_reference.py, pinned against Pillow's outputs in tests/golden/rectify_pillow.npz):
//   output pixel (x, y), xin = x + 0.5, yin = y + 0.5, in DOUBLE without contraction, both divisions correctly rounded:
//     sx = (a0 xin + a1 yin + a2) / (a6 xin + a7 yin + 1),   sy = (a3 xin + a4 yin + a5) / (a6 xin + a7 yin + 1)
//   the pixel stays 0 unless 0 <= sx < W and 0 <= sy < H (written so that NaN is outside); otherwise the sixteen taps of
//   aug_bicubic_taps (augment.h) around floor(sx - 0.5), floor(sy - 0.5).
// ONE launch rectifies all regions of a call: grid = the tiles (RECT_TILE x RECT_TILE output pixels) of all regions, a workgroup finds its
// region by bisection in the prefix sums of the tile counts, a work-item produces one pixel's three channels.  rectify_plan_kernel builds
// those prefix sums, places the ragged outputs (slots of 3 w h bytes, 256-byte aligned, or the caller's own buffers) and writes the ImageDesc
// array resize_bicubic_kernel (resize.h) then reads — all on the device, so no host array of the library's has to outlive the call.
// Nothing is staged in LDS: a tile's taps cover a few KB of the source around one spot, which the CU's vector cache and L2 serve; the
// arithmetic (about 130 double operations a pixel) is small against the launch and the gather (measured in profiles/rectify.md).
// Every source index is clamped to the image the host validated, and a pixel outside its region's size leaves at once.
#pragma once
#include "augment.h"

namespace pq {

constexpr int RECT_TILE = 16;                        // 16 x 16 output pixels = the 256 work-items of a workgroup
constexpr int RECT_MAX_TILES = 1 << 23;              // of one call: 2^31 work-items, half of what a launch can hold

struct RegionDesc { int image, height, width; double coef[8]; };          // mirrors parseq_region_desc

__host__ __device__ inline int rect_tiles(int h, int w) { return ((h + RECT_TILE - 1) / RECT_TILE) * ((w + RECT_TILE - 1) / RECT_TILE); }
__host__ __device__ inline size_t rect_slot_bytes(int h, int w) { return ((size_t)h * (size_t)w * 3 + 255) & ~(size_t)255; }

// tile_start[i] = first tile of region i (tile_start[n] = all tiles); dst[i] = where region i is written: outs[i] if the caller brought
// buffers, else its slot; finals[i] = the rectified region as an image for the resize.  Region is any descriptor with a height and a width
// (RegionDesc here, MeshRegionDesc in rectify_mesh.h).
template <class Region>
static __global__ __launch_bounds__(256)
void rectify_plan_kernel(const Region* __restrict__ regions, int n, unsigned char* const* __restrict__ outs, unsigned char* slots,
                         int* __restrict__ tile_start, unsigned char** __restrict__ dst, ImageDesc* __restrict__ finals) {
    __shared__ int st[256];
    __shared__ unsigned long long sb[256];
    const int tid = threadIdx.x;
    int tiles_before = 0;
    unsigned long long bytes_before = 0;
    for (int base = 0; base < n; base += 256) {                           // an inclusive scan of 256 regions at a time
        const int i = base + tid;
        int h = 0, w = 0, t = 0;
        unsigned long long b = 0;
        if (i < n) { h = regions[i].height; w = regions[i].width; t = rect_tiles(h, w); b = rect_slot_bytes(h, w); }
        st[tid] = t; sb[tid] = b;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int tv = tid >= off ? st[tid - off] : 0;
            const unsigned long long bv = tid >= off ? sb[tid - off] : 0;
            __syncthreads();
            st[tid] += tv; sb[tid] += bv;
            __syncthreads();
        }
        if (i < n) {
            tile_start[i] = tiles_before + st[tid] - t;
            unsigned char* d = outs ? outs[i] : slots + (size_t)(bytes_before + sb[tid] - b);
            dst[i] = d;
            ImageDesc f;
            f.data = d; f.height = h; f.width = w; f.row_stride = 3LL * w;
            finals[i] = f;
        }
        tiles_before += st[255]; bytes_before += sb[255];
        __syncthreads();                                                   // the next 256 regions overwrite st / sb
    }
    if (tid == 0) tile_start[n] = tiles_before;
}

// the tail every Image.transform map shares: the inside test and the bicubic taps around the source position (sx, sy); false where the fill stays
__device__ __forceinline__ bool rect_sample(const unsigned char* src, long long stride, int h, int w, double sx, double sy, unsigned char* out) {
    int fx, fy;
    double dx, dy;
    if (!aug_source_pixel(sx, sy, h, w, &fx, &fy, &dx, &dy)) return false;
    aug_bicubic_taps(src, stride, h, w, fx, fy, dx, dy, out);
    return true;
}

// one output pixel of Image.transform(PERSPECTIVE, BICUBIC): false where the fill stays
__device__ __forceinline__ bool rect_pixel(const unsigned char* src, long long stride, int h, int w, const double* a, int x, int y, unsigned char* out) {
    AUG_NO_CONTRACT
    const double xin = (double)x + 0.5, yin = (double)y + 0.5;
    const double den = AUG_ADD(AUG_ADD(AUG_MUL(a[6], xin), AUG_MUL(a[7], yin)), 1.0);
    const double sx = AUG_DIV(AUG_ADD(AUG_ADD(AUG_MUL(a[0], xin), AUG_MUL(a[1], yin)), a[2]), den);
    const double sy = AUG_DIV(AUG_ADD(AUG_ADD(AUG_MUL(a[3], xin), AUG_MUL(a[4], yin)), a[5]), den);
    return rect_sample(src, stride, h, w, sx, sy, out);
}

// The front of every rectification kernel: workgroup blockIdx.x is a tile of region *region (bisection in tile_start), the work-item is pixel
// (*x, *y) of that region.  False for a workgroup beyond the tiles and for a pixel outside the region's size.
template <class Region>
__device__ __forceinline__ bool rect_locate(const Region* __restrict__ regions, int n, const int* __restrict__ tile_start, int* region, int* x, int* y) {
    const int b = blockIdx.x;
    if (b >= tile_start[n]) return false;
    int lo = 0, hi = n;                                                    // tile_start[lo] <= b < tile_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_start[mid] <= b) lo = mid; else hi = mid;
    }
    const int oh = regions[lo].height, ow = regions[lo].width;
    const int t = b - tile_start[lo];
    const int across = (ow + RECT_TILE - 1) / RECT_TILE;
    const int ty = t / across, tx = t - ty * across;
    *region = lo;
    *x = tx * RECT_TILE + (int)(threadIdx.x % RECT_TILE); *y = ty * RECT_TILE + (int)(threadIdx.x / RECT_TILE);
    return *x < ow && *y < oh;
}

// their tail: pixel (x, y) of a region ow wide, HWC and tight at `out`: v, or 0 where the fill stays
__device__ __forceinline__ void rect_store(unsigned char* out, int ow, int x, int y, bool inside, const unsigned char* v) {
    unsigned char* o = out + ((size_t)y * (size_t)ow + (size_t)x) * 3;
    o[0] = inside ? v[0] : 0; o[1] = inside ? v[1] : 0; o[2] = inside ? v[2] : 0;
}

// grid = tile_start[n] workgroups.  Region i is written HWC, tight, at dst[i].
static __global__ __launch_bounds__(256)
void rectify_kernel(const ImageDesc* __restrict__ images, int n_images, const RegionDesc* __restrict__ regions, int n,
                    const int* __restrict__ tile_start, unsigned char* const* __restrict__ dst) {
    int i, x, y;
    if (!rect_locate(regions, n, tile_start, &i, &x, &y)) return;
    const RegionDesc& r = regions[i];
    if ((unsigned)r.image >= (unsigned)n_images) return;                   // never, for descriptors the host accepted
    const ImageDesc im = images[r.image];
    double a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = r.coef[k];
    unsigned char v[3];
    const bool inside = rect_pixel(im.data, im.row_stride, im.height, im.width, a, x, y, v);
    rect_store(dst[i], r.width, x, y, inside, v);
}

}  // namespace pq
