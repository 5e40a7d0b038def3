// Rectification of polygon text regions on the device: what a caller with a detector of curved text does first.
// A region (image index, output size, a run of strips) is a row of strips side by side; strip k owns the output columns x0 .. x1 - 1 and
// reads the region's source image through the bilinear map of one quadrilateral, byte for byte
// Image.transform((w, h), Image.MESH, [((x0, 0, x1, h), quad), ...], Image.BICUBIC) with fill 0 (restated in tests/mesh_reference.py,
// pinned against Pillow's outputs in tests/golden/mesh_pillow.npz):
//   output pixel (x, y) of the strip with x0 <= x < x1, xin = (x - x0) + 0.5, yin = y + 0.5, in DOUBLE without contraction, left to right:
//     sx = a0 + a1 xin + a2 yin + a3 xin yin,   sy = a4 + a5 xin + a6 yin + a7 xin yin
//   then the inside test and the sixteen taps of rectify.h (rect_sample), which this kernel shares with rectify_kernel.
// ONE launch for all regions of a call, planned by rectify.h's rectify_plan_kernel: grid = the RECT_TILE x RECT_TILE tiles of all regions,
// a workgroup finds its region by bisection in the tile table, a work-item produces one pixel's three channels.
// The strip of a pixel is found in the strip table in GLOBAL memory, with integers only: the workgroup bisects for the strip of its tile's
// first column — the same for every lane, so these are scalar loads — and each lane then steps right while its column is at or beyond its
// strip's x1: at most 15 steps, since every strip is at least one column wide, and none or one for strips as wide as a tile.  Staging the
// tile's strips in LDS instead would cost a barrier and a second pass over the same 72-byte records to save loads that the scalar and
// vector caches already serve (a region's whole table is at most 64 x 72 bytes = 4.5 KB); the map itself is 8 double multiplications
// and 6 additions a pixel, without the two divisions of the perspective map, against sixteen gathered taps.  The lookup depends on the
// pixel's column and the region's table alone, so the result does not depend on the tile size or on the grid.
// Every strip index stays inside the run [first_strip, first_strip + n_strips) the host validated (it tiles [0, width) exactly), every
// source index is clamped to the image, and a pixel outside its region's size leaves at once.
#pragma once
#include "rectify.h"

namespace pq {

constexpr int MESH_MAX_STRIPS = 64;                  // PARSEQ_MESH_MAX_STRIPS

struct MeshStrip { int x0, x1; double coef[8]; };                          // mirrors parseq_mesh_strip
struct MeshRegionDesc { int image, height, width, first_strip, n_strips; };  // mirrors parseq_mesh_region_desc

// one output pixel of a strip of Image.transform(MESH, BICUBIC): xrel = the column within the strip; false where the fill stays
__device__ __forceinline__ bool mesh_pixel(const unsigned char* src, long long stride, int h, int w, const double* a, int xrel, int y, unsigned char* out) {
    AUG_NO_CONTRACT
    const double xin = (double)xrel + 0.5, yin = (double)y + 0.5;
    const double sx = AUG_ADD(AUG_ADD(AUG_ADD(a[0], AUG_MUL(a[1], xin)), AUG_MUL(a[2], yin)), AUG_MUL(AUG_MUL(a[3], xin), yin));
    const double sy = AUG_ADD(AUG_ADD(AUG_ADD(a[4], AUG_MUL(a[5], xin)), AUG_MUL(a[6], yin)), AUG_MUL(AUG_MUL(a[7], xin), yin));
    return rect_sample(src, stride, h, w, sx, sy, out);
}

// grid = tile_start[n] workgroups.  Region i is written HWC, tight, at dst[i].
static __global__ __launch_bounds__(256)
void mesh_rectify_kernel(const ImageDesc* __restrict__ images, int n_images, const MeshRegionDesc* __restrict__ regions, int n,
                         const MeshStrip* __restrict__ strips, const int* __restrict__ tile_start, unsigned char* const* __restrict__ dst) {
    int i, x, y;
    if (!rect_locate(regions, n, tile_start, &i, &x, &y)) return;
    const MeshRegionDesc r = regions[i];
    const int ns = r.n_strips;
    if ((unsigned)r.image >= (unsigned)n_images || ns < 1 || ns > MESH_MAX_STRIPS) return;    // never, for descriptors the host accepted
    const MeshStrip* st = strips + r.first_strip;
    // the tile's first column: the same for every lane, and taken from the first so that the bisection below runs on scalar loads
    const int tile_x = __builtin_amdgcn_readfirstlane(x) / RECT_TILE * RECT_TILE;
    int k = 0, kh = ns;                                                    // st[k].x0 <= the tile's first column < st[kh].x0 (st[ns].x0 = ow)
    while (kh - k > 1) {
        const int mid = (k + kh) >> 1;
        if (st[mid].x0 <= tile_x) k = mid; else kh = mid;
    }
    while (k + 1 < ns && x >= st[k].x1) ++k;
    const ImageDesc im = images[r.image];
    double a[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) a[c] = st[k].coef[c];
    unsigned char v[3];
    const bool inside = mesh_pixel(im.data, im.row_stride, im.height, im.width, a, x - st[k].x0, y, v);
    rect_store(dst[i], r.width, x, y, inside, v);
}

}  // namespace pq
