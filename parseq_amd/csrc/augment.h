// The RandAugment operators of the reference's training transform on the device (strhub/data/augment.py, aa_overrides.py:
// timm's auto_augment operators, i.e. calls into Pillow), bit-exact with Pillow on RGB images (restated in
// tests/augment_reference.py, pinned against Pillow's outputs in tests/golden/augment_pillow.npz).
//
// A chain of up to three operators per image runs stage by stage over the whole ragged batch: stage k is ONE launch, grid =
// images x tiles, and an image whose chain is shorter than k + 1 leaves at once.  Stage 0 reads the caller's image, every
// stage writes one of two per-image regions of the workspace (ping-pong), so the image after its last operator is the source
// itself (empty chain), region 0 (one or three operators) or region 1 (two); nothing is ever copied through.
// augment_plan_kernel places the regions and writes the ImageDesc array that resize_bicubic_kernel (resize.h) then reads.
//
// Operators (the Python half, parseq_amd/augment.py, maps the reference's sixteen names onto them):
//   AUG_TABLE         Invert, Posterize, Solarize, SolarizeAdd, Brightness: a 256-entry table built on the host, one pass;
//   AUG_AUTOCONTRAST  per-channel histogram -> ImageOps.autocontrast's table (float64, no fused multiply-add);
//   AUG_EQUALIZE      per-channel histogram -> ImageOps.equalize's table (integers);
//   AUG_CONTRAST      sum of L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16 -> rounded mean -> table of Image.blend(mean, v, f);
//   AUG_COLOR         Image.blend(L of the pixel, pixel, f): not a table, L differs per pixel;
//   AUG_AFFINE        Image.transform(AFFINE, BILINEAR | BICUBIC, fillcolor 128): ShearX/Y, TranslateX/YRel and Rotate(expand);
//   AUG_TURN          Rotate by 90 / 180 / 270 degrees: Pillow's exact transposes, whatever the filter;
//   AUG_GAUSSIAN_BLUR Image.filter(ImageFilter.GaussianBlur(radius)): Pillow's three box passes along x, then three along y, in 8.24
//                     fixed point (aug_blur_tiles below); the host half gaussian_box(radius) gives the pass's (r, ww, fw);
//   AUG_POISSON_NOISE imgaug's AdditivePoissonNoise(lam), restated: n = +-k, k ~ Poisson(lam), one draw per pixel added to R, G and B and
//                     clipped; Philox4x32-10 keyed by the seed, counter = the pixel's index, thresholds in float64 (aug_noise_table below).
// Statistics are gathered in LDS with integer atomics (exact, order-independent: the same bytes every run), the table is built in
// LDS and applied in the same launch.  An image of more than one tile gathers its statistics once per tile (each workgroup reads
// the whole image, at most AUG_MAX_TILES times, from L2) — no grid-wide synchronisation, no second launch.
// Image.blend computes in SINGLE precision, the affine map and its taps in DOUBLE; both without contraction.  The *_rn intrinsics do
// not give that (AutoContrast's int(ix * scale + offset) was one off on an MI355X that way), so every function below that does
// floating-point arithmetic opens with AUG_NO_CONTRACT and uses the plain-operator macros of resize.h, where the reason is told: none of
// its operations carries the `contract` flag, wherever they end up inlined (checked in the unit's LLVM IR: no fmul / fadd of
// augment_stage_kernel has `contract`).
#pragma once
#include "resize.h"

namespace pq {

// 9 is no operator: tests/test_augment.py holds the library to refusing it
enum { AUG_NONE = 0, AUG_TABLE = 1, AUG_AUTOCONTRAST = 2, AUG_EQUALIZE = 3, AUG_CONTRAST = 4, AUG_COLOR = 5, AUG_AFFINE = 6, AUG_TURN = 7,
       AUG_GAUSSIAN_BLUR = 8, AUG_POISSON_NOISE = 10 };
enum { AUG_BILINEAR = 2, AUG_BICUBIC = 3 };          // Pillow's Image.Resampling values
constexpr int AUG_MAX_OPS = 3;
constexpr int AUG_TILE_PIXELS = 4096;                // pixels of one workgroup's share, until an image has AUG_MAX_TILES of them
constexpr int AUG_MAX_TILES = 16;
constexpr int AUG_FILL = 128;
constexpr int AUG_BLUR_MAX_R = 3;                    // the box radius of GaussianBlur(4), the policy's largest
constexpr int AUG_BLUR_TILE_H = 32, AUG_BLUR_TILE_W = 64;                         // outputs of one sub-tile of the blur
constexpr int AUG_BLUR_MAX_HALO = 3 * (AUG_BLUR_MAX_R + 1);                      // three passes, each reaching r + 1 samples
constexpr int AUG_BLUR_PLANE = (AUG_BLUR_TILE_H + 2 * AUG_BLUR_MAX_HALO) * (AUG_BLUR_TILE_W + 2 * AUG_BLUR_MAX_HALO) * 3;    // 14784 bytes
constexpr int AUG_NOISE_MAX_LAM = 41;
constexpr int AUG_NOISE_LEVELS = 127;                // thresholds T_0 .. T_126: k <= 127

struct AugOp {                                       // mirrors parseq_augment_op
    int op, mode, out_height, out_width;
    union {
        unsigned char table[256]; float factor; double coef[6];
        struct { int r; unsigned ww, fw; } blur;
        struct { double p0; unsigned long long seed; int lam; } noise;
    } arg;
};
struct AugDesc {                                     // mirrors parseq_augment_desc
    const unsigned char* data; int height, width; long long row_stride;
    int num_ops, reserved;
    AugOp ops[AUG_MAX_OPS];
};

__host__ __device__ inline int aug_tiles(long long pixels) {
    const long long t = (pixels + AUG_TILE_PIXELS - 1) / AUG_TILE_PIXELS;
    return t < 1 ? 1 : (t > AUG_MAX_TILES ? AUG_MAX_TILES : (int)t);
}

// bytes of ONE of an image's two regions: its largest stage output, rounded up to 256
template <class D> __host__ __device__ inline size_t aug_region_bytes(const D& d) {
    size_t most = 0;
    for (int k = 0; k < d.num_ops && k < AUG_MAX_OPS; ++k) {
        const size_t b = (size_t)d.ops[k].out_height * (size_t)d.ops[k].out_width * 3;
        most = b > most ? b : most;
    }
    return (most + 255) & ~(size_t)255;
}

// offsets[i] = start of image i's pair of regions; finals[i] = the image after its last operator
static __global__ __launch_bounds__(256)
void augment_plan_kernel(const AugDesc* __restrict__ descs, int n, unsigned char* regions, size_t* offsets, ImageDesc* finals) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) offsets[i] = 2 * aug_region_bytes(descs[i]);
    __syncthreads();
    if (threadIdx.x == 0) {
        size_t at = 0;
        for (int i = 0; i < n; ++i) { const size_t b = offsets[i]; offsets[i] = at; at += b; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const AugDesc& d = descs[i];
        ImageDesc f;
        if (d.num_ops == 0) {
            f.data = d.data; f.height = d.height; f.width = d.width; f.row_stride = d.row_stride;
        } else {
            const AugOp& last = d.ops[d.num_ops - 1];
            f.data = regions + offsets[i] + (size_t)((d.num_ops - 1) & 1) * aug_region_bytes(d);
            f.height = last.out_height; f.width = last.out_width; f.row_stride = 3LL * last.out_width;
        }
        finals[i] = f;
    }
}

// Pillow's ImagingBlend for one sample: a = degenerate, b = image, f = factor (never 0 here: the host refuses f < 0.1)
__device__ __forceinline__ unsigned char aug_blend(int a, int b, float f) {
    AUG_NO_CONTRACT
    if (f == 1.0f) return (unsigned char)b;
    const float t = (float)a + f * (float)(b - a);
    if (f <= 1.0f) return (unsigned char)(int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (unsigned char)(int)t);
}

__device__ __forceinline__ int aug_luma(const unsigned char* p) {
    return (int)(((unsigned)p[0] * 19595u + (unsigned)p[1] * 38470u + (unsigned)p[2] * 7471u + 0x8000u) >> 16);
}

// Pillow's BICUBIC(v, v1, v2, v3, v4, d) of Geometry.c, in its order of operations
__device__ __forceinline__ double aug_cubic(double v1, double v2, double v3, double v4, double d) {
    AUG_NO_CONTRACT
    const double p2 = AUG_ADD(-v1, v3);
    const double p3 = AUG_ADD(AUG_ADD(AUG_MUL(2.0, AUG_ADD(v1, -v2)), v3), -v4);
    const double p4 = AUG_ADD(AUG_ADD(AUG_ADD(-v1, v2), -v3), v4);
    return AUG_ADD(v2, AUG_MUL(d, AUG_ADD(p2, AUG_MUL(d, AUG_ADD(p3, AUG_MUL(d, p4))))));
}

__device__ __forceinline__ int aug_clampi(int v, int n) { return v < 0 ? 0 : (v < n ? v : n - 1); }

// Pillow's bicubic_filter32RGB around source pixel (fx, fy) with the fractions (dx, dy): sixteen clamped taps, a row outside the image
// repeating the value of the row above, clipped and truncated.  Shared by the affine operator below and the projective map of rectify.h.
__device__ __forceinline__ void aug_bicubic_taps(const unsigned char* src, long long stride, int h, int w, int fx, int fy, double dx, double dy,
                                                 unsigned char* out) {
    AUG_NO_CONTRACT
    size_t xs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) xs[t] = (size_t)aug_clampi(fx - 1 + t, w) * 3;
    const unsigned char* rows[4];
    bool has[4];
    rows[0] = src + (size_t)aug_clampi(fy - 1, h) * stride; has[0] = true;
#pragma unroll
    for (int t = 1; t < 4; ++t) {
        const int yy = fy - 1 + t;
        has[t] = yy >= 0 && yy < h;
        rows[t] = src + (size_t)(has[t] ? yy : 0) * stride;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v[4];
        v[0] = aug_cubic(rows[0][xs[0] + c], rows[0][xs[1] + c], rows[0][xs[2] + c], rows[0][xs[3] + c], dx);
#pragma unroll
        for (int t = 1; t < 4; ++t) {
            if (has[t]) v[t] = aug_cubic(rows[t][xs[0] + c], rows[t][xs[1] + c], rows[t][xs[2] + c], rows[t][xs[3] + c], dx);
            else v[t] = v[t - 1];                  // a missing row repeats the value of the row above
        }
        const double r = aug_cubic(v[0], v[1], v[2], v[3], dy);
        out[c] = r <= 0.0 ? 0 : (r >= 255.0 ? 255 : (unsigned char)(int)r);
    }
}

// Where the source position (sx, sy) of an Image.transform map falls in an h x w image: false outside (written so that NaN is outside), where the
// fill stays; else the pixel (*fx, *fy) = the floor of the position half a pixel back, and the fractions (*dx, *dy) beyond it
__device__ __forceinline__ bool aug_source_pixel(double sx, double sy, int h, int w, int* fx, int* fy, double* dx, double* dy) {
    AUG_NO_CONTRACT
    if (!(sx >= 0.0 && sx < (double)w && sy >= 0.0 && sy < (double)h)) return false;
    sx = AUG_ADD(sx, -0.5); sy = AUG_ADD(sy, -0.5);
    *fx = (int)floor(sx); *fy = (int)floor(sy);
    *dx = AUG_ADD(sx, -(double)*fx); *dy = AUG_ADD(sy, -(double)*fy);
    return true;
}

// one output pixel of Image.transform(AFFINE): false where the fill colour stays
__device__ __forceinline__ bool aug_affine_pixel(const unsigned char* src, long long stride, int h, int w, const double* a, int resample,
                                                 int x, int y, unsigned char* out) {
    AUG_NO_CONTRACT
    const double xin = (double)x + 0.5, yin = (double)y + 0.5;
    const double sx = AUG_ADD(AUG_ADD(AUG_MUL(a[0], xin), AUG_MUL(a[1], yin)), a[2]);
    const double sy = AUG_ADD(AUG_ADD(AUG_MUL(a[3], xin), AUG_MUL(a[4], yin)), a[5]);
    int fx, fy;
    double dx, dy;
    if (!aug_source_pixel(sx, sy, h, w, &fx, &fy, &dx, &dy)) return false;
    if (resample == AUG_BILINEAR) {
        const size_t x0 = (size_t)aug_clampi(fx, w) * 3, x1 = (size_t)aug_clampi(fx + 1, w) * 3;
        const unsigned char* r0 = src + (size_t)aug_clampi(fy, h) * stride;
        const bool has1 = fy + 1 >= 0 && fy + 1 < h;
        const unsigned char* r1 = src + (size_t)(has1 ? fy + 1 : 0) * stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p = r0[x0 + c], q = r0[x1 + c];
            const double v1 = AUG_ADD(p, AUG_MUL(AUG_ADD(q, -p), dx));
            double v2 = v1;
            if (has1) { const double p2 = r1[x0 + c], q2 = r1[x1 + c]; v2 = AUG_ADD(p2, AUG_MUL(AUG_ADD(q2, -p2), dx)); }
            out[c] = (unsigned char)(int)AUG_ADD(v1, AUG_MUL(AUG_ADD(v2, -v1), dy));
        }
    } else {
        aug_bicubic_taps(src, stride, h, w, fx, fy, dx, dy, out);
    }
    return true;
}

// ---- GaussianBlur: Pillow's BoxBlur.c ------------------------------------------------------------------------------------------
// One box pass over the lh x lw x 3 bytes of a tile in LDS, along x or along y:
//   out = (ww * sum(in[clamp(. + i)], i = -r .. r) + fw * (in[clamp(. - r - 1)] + in[clamp(. + r + 1)]) + 2^23) >> 24,   32-bit unsigned
// (the host refuses (2 r + 1) ww + 2 fw > 2^24, so nothing wraps).  Indices are clamped to the TILE: where the tile ends at the image's
// edge that is Pillow's clamp, applied to this pass's own input; where it ends inside the image the samples are wrong, r + 1 deeper
// with every pass — the halo of 3 (r + 1) that is never written back.
template <bool ALONG_X>
__device__ __forceinline__ void aug_box_pass(const unsigned char* in, unsigned char* out, int lh, int lw, int r, unsigned ww, unsigned fw, int tid) {
    const int row = lw * 3, n = lh * row;
    for (int e = tid; e < n; e += 256) {
        const int y = e / row, xc = e - y * row;
        unsigned acc = 0, far;
        if (ALONG_X) {
            const int x = xc / 3;
            const unsigned char* line = in + y * row + (xc - x * 3);
            for (int i = -r; i <= r; ++i) acc += line[aug_clampi(x + i, lw) * 3];
            far = (unsigned)line[aug_clampi(x - r - 1, lw) * 3] + line[aug_clampi(x + r + 1, lw) * 3];
        } else {
            const unsigned char* line = in + xc;
            for (int i = -r; i <= r; ++i) acc += line[aug_clampi(y + i, lh) * row];
            far = (unsigned)line[aug_clampi(y - r - 1, lh) * row] + line[aug_clampi(y + r + 1, lh) * row];
        }
        out[e] = (unsigned char)((acc * ww + far * fw + (1u << 23)) >> 24);
    }
}

// The workgroup's share [p0, p1) of an h x w image, walked in sub-tiles of AUG_BLUR_TILE_H x AUG_BLUR_TILE_W outputs: each is loaded with its
// halo (cut at the image's edges), runs the six passes between the two planes in LDS and writes the pixels of the share.  Every branch
// is uniform over the workgroup.
__device__ __forceinline__ void aug_blur_tiles(const unsigned char* src, long long stride, int h, int w, unsigned char* dst, int p0, int p1,
                                               int r, unsigned ww, unsigned fw, unsigned char* a, unsigned char* b, int tid) {
    const int halo = 3 * (r + 1);
    const int y0 = p0 / w, y1 = (p1 - 1) / w + 1;
    for (int ty0 = y0; ty0 < y1; ty0 += AUG_BLUR_TILE_H) {
        const int ty1 = min(y1, ty0 + AUG_BLUR_TILE_H);
        const int gy0 = max(0, ty0 - halo), lh = min(h, ty1 + halo) - gy0;
        for (int tx0 = 0; tx0 < w; tx0 += AUG_BLUR_TILE_W) {
            const int tx1 = min(w, tx0 + AUG_BLUR_TILE_W);
            if ((ty1 - 1) * w + tx1 - 1 < p0 || ty0 * w + tx0 >= p1) continue;                // no pixel of the share in this sub-tile
            const int gx0 = max(0, tx0 - halo), lw = min(w, tx1 + halo) - gx0;
            const int row = lw * 3, n = lh * row;
            for (int e = tid; e < n; e += 256) {
                const int y = e / row, xc = e - y * row;
                a[e] = src[(size_t)(gy0 + y) * stride + (size_t)gx0 * 3 + xc];
            }
            __syncthreads();
            aug_box_pass<true>(a, b, lh, lw, r, ww, fw, tid);  __syncthreads();
            aug_box_pass<true>(b, a, lh, lw, r, ww, fw, tid);  __syncthreads();
            aug_box_pass<true>(a, b, lh, lw, r, ww, fw, tid);  __syncthreads();
            aug_box_pass<false>(b, a, lh, lw, r, ww, fw, tid); __syncthreads();
            aug_box_pass<false>(a, b, lh, lw, r, ww, fw, tid); __syncthreads();
            aug_box_pass<false>(b, a, lh, lw, r, ww, fw, tid); __syncthreads();
            const int tw = tx1 - tx0, outs = (ty1 - ty0) * tw;
            for (int e = tid; e < outs; e += 256) {
                const int ly = e / tw, y = ty0 + ly, x = tx0 + (e - ly * tw);
                const int p = y * w + x;
                if (p < p0 || p >= p1) continue;
                const unsigned char* px = a + ((y - gy0) * lw + (x - gx0)) * 3;
                unsigned char* o = dst + (size_t)p * 3;
                o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
            }
            __syncthreads();                                                                 // the next sub-tile loads into `a`
        }
    }
}

// ---- PoissonNoise ------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11; Random123), counter (c0, c1, 0, 0), key (k0, k1): words 0 and 1 of the output
__device__ __forceinline__ void aug_philox(unsigned c0, unsigned c1, unsigned k0, unsigned k1, unsigned& w0, unsigned& w1) {
    unsigned c2 = 0, c3 = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long m0 = 0xD2511F53ull * c0, m1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(m1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(m0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)m1; c3 = (unsigned)m0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w0 = c0; w1 = c1;
}

// T_j = min(floor(C_j 2^32), 2^32 - 1), C_j = C_{j-1} + p_j, p_{j+1} = (p_j lam) / (j + 1), p_0 = exp(-lam) from the host: float64, one
// thread, in this order.  k of a uniform u is the number of T_j <= u.
__device__ __forceinline__ void aug_noise_table(unsigned* T, double p0, int lam) {
    AUG_NO_CONTRACT
    double p = p0, c = p0;
    const double dl = (double)lam;
    for (int j = 0; j < AUG_NOISE_LEVELS; ++j) {
        const double t = AUG_MUL(c, 4294967296.0);
        T[j] = t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
        p = AUG_MUL(p, dl) / (double)(j + 1);
        c = AUG_ADD(c, p);
    }
}

// stage k of every image's chain.  grid = (images, most tiles of an image at this stage)
static __global__ __launch_bounds__(256)
void augment_stage_kernel(const AugDesc* __restrict__ descs, const size_t* __restrict__ offsets, unsigned char* regions, int k) {
    AUG_NO_CONTRACT
    __shared__ unsigned hist[768];
    __shared__ unsigned char lut[768];
    __shared__ unsigned long long lsum;
    __shared__ int lohi[6];
    __shared__ unsigned char blur[2][AUG_BLUR_PLANE];
    const AugDesc& d = descs[blockIdx.x];
    if (k >= d.num_ops) return;
    const AugOp& op = d.ops[k];
    const int h = k ? d.ops[k - 1].out_height : d.height, w = k ? d.ops[k - 1].out_width : d.width;
    const int oh = op.out_height, ow = op.out_width;
    const int opx = oh * ow;
    const int tiles = aug_tiles(opx);
    if ((int)blockIdx.y >= tiles) return;
    const size_t region = aug_region_bytes(d);
    unsigned char* base = regions + offsets[blockIdx.x];
    const unsigned char* src = k ? base + (size_t)((k - 1) & 1) * region : d.data;
    const long long stride = k ? 3LL * w : d.row_stride;
    unsigned char* dst = base + (size_t)(k & 1) * region;
    const int chunk = (opx + tiles - 1) / tiles;
    const int p0 = (int)blockIdx.y * chunk, p1 = min(opx, p0 + chunk);
    if (p0 >= p1) return;
    const int tid = threadIdx.x;
    const int kind = op.op;

    if (kind == AUG_AUTOCONTRAST || kind == AUG_EQUALIZE || kind == AUG_CONTRAST) {          // statistics of the WHOLE image (h x w = oh x ow)
        for (int t = tid; t < 768; t += blockDim.x) hist[t] = 0;
        if (tid == 0) lsum = 0;
        __syncthreads();
        const int npx = h * w;
        if (kind == AUG_CONTRAST) {
            unsigned long long part = 0;
            for (int p = tid; p < npx; p += blockDim.x) { const int y = p / w, x = p - y * w; part += (unsigned)aug_luma(src + (size_t)y * stride + (size_t)x * 3); }
            atomicAdd(&lsum, part);
        } else {
            for (int p = tid; p < npx; p += blockDim.x) {
                const int y = p / w, x = p - y * w;
                const unsigned char* px = src + (size_t)y * stride + (size_t)x * 3;
                atomicAdd(&hist[px[0]], 1u); atomicAdd(&hist[256 + px[1]], 1u); atomicAdd(&hist[512 + px[2]], 1u);
            }
        }
        __syncthreads();
        if (kind == AUG_CONTRAST) {
            const int mean = (int)AUG_ADD(((double)lsum / (double)npx), 0.5);
            const float f = op.arg.factor;
            for (int t = tid; t < 768; t += blockDim.x) lut[t] = aug_blend(mean, t & 255, f);
        } else if (kind == AUG_AUTOCONTRAST) {
            if (tid < 3) {
                const unsigned* hc = hist + 256 * tid;
                int lo = 0, hi = 255;
                while (lo < 255 && !hc[lo]) ++lo;
                while (hi > 0 && !hc[hi]) --hi;
                lohi[2 * tid] = lo; lohi[2 * tid + 1] = hi;
            }
            __syncthreads();
            for (int t = tid; t < 768; t += blockDim.x) {
                const int lo = lohi[2 * (t >> 8)], hi = lohi[2 * (t >> 8) + 1], ix = t & 255;
                int v = ix;
                if (hi > lo) {
                    const double scale = 255.0 / (double)(hi - lo);
                    const double offset = AUG_MUL(-(double)lo, scale);
                    v = (int)AUG_ADD(AUG_MUL((double)ix, scale), offset);
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                }
                lut[t] = (unsigned char)v;
            }
        } else if (tid < 3) {                                                                // ImageOps.equalize, one channel per thread
            const unsigned* hc = hist + 256 * tid;
            unsigned char* lc = lut + 256 * tid;
            long long total = 0, last = 0;
            int levels = 0;
            for (int i = 0; i < 256; ++i) if (hc[i]) { total += hc[i]; last = hc[i]; ++levels; }
            const long long step = (total - last) / 255;
            if (levels <= 1 || step == 0) {
                for (int i = 0; i < 256; ++i) lc[i] = (unsigned char)i;
            } else {
                long long n = step / 2;
                for (int i = 0; i < 256; ++i) { const long long v = n / step; lc[i] = (unsigned char)(v > 255 ? 255 : v); n += hc[i]; }
            }
        }
        __syncthreads();
    } else if (kind == AUG_TABLE) {
        for (int t = tid; t < 768; t += blockDim.x) lut[t] = op.arg.table[t & 255];
        __syncthreads();
    } else if (kind == AUG_POISSON_NOISE) {                                                  // the thresholds take hist's place
        if (tid == 0) aug_noise_table(hist, op.arg.noise.p0, op.arg.noise.lam);
        __syncthreads();
    }

    if (kind == AUG_AFFINE) {
        double a[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) a[t] = op.arg.coef[t];
        const int resample = op.mode;
        for (int p = p0 + tid; p < p1; p += blockDim.x) {
            const int y = p / ow, x = p - y * ow;
            unsigned char v[3];
            if (!aug_affine_pixel(src, stride, h, w, a, resample, x, y, v)) v[0] = v[1] = v[2] = AUG_FILL;
            unsigned char* o = dst + (size_t)p * 3;
            o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
        }
    } else if (kind == AUG_TURN) {
        const int mode = op.mode;
        for (int p = p0 + tid; p < p1; p += blockDim.x) {
            const int y = p / ow, x = p - y * ow;
            int sx, sy;
            if (mode == ROT_90) { sx = w - 1 - y; sy = x; }
            else if (mode == ROT_180) { sx = w - 1 - x; sy = h - 1 - y; }
            else { sx = y; sy = h - 1 - x; }
            unsigned char* o = dst + (size_t)p * 3;
            if ((unsigned)sx < (unsigned)w && (unsigned)sy < (unsigned)h) {                  // always, for a descriptor the host accepted
                const unsigned char* px = src + (size_t)sy * stride + (size_t)sx * 3;
                o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
            } else { o[0] = o[1] = o[2] = AUG_FILL; }
        }
    } else if (kind == AUG_GAUSSIAN_BLUR) {
        aug_blur_tiles(src, stride, h, w, dst, p0, p1, min(max(op.arg.blur.r, 0), AUG_BLUR_MAX_R), op.arg.blur.ww, op.arg.blur.fw, blur[0], blur[1], tid);
    } else if (kind == AUG_POISSON_NOISE) {
        const unsigned k0 = (unsigned)op.arg.noise.seed, k1 = (unsigned)(op.arg.noise.seed >> 32);
        for (int p = p0 + tid; p < p1; p += blockDim.x) {
            const int y = p / ow, x = p - y * ow;
            unsigned u, sign;
            aug_philox((unsigned)p, 0u, k0, k1, u, sign);                                    // the pixel's index is below 2^31: its high word is 0
            int lo = 0, hi = AUG_NOISE_LEVELS;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (hist[mid] <= u) lo = mid + 1; else hi = mid; }
            const int n = (sign >> 31) ? -lo : lo;
            const unsigned char* px = src + (size_t)y * stride + (size_t)x * 3;
            unsigned char* o = dst + (size_t)p * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) { const int v = (int)px[c] + n; o[c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
        }
    } else if (kind == AUG_COLOR) {
        const float f = op.arg.factor;
        for (int p = p0 + tid; p < p1; p += blockDim.x) {
            const int y = p / ow, x = p - y * ow;
            const unsigned char* px = src + (size_t)y * stride + (size_t)x * 3;
            const int l = aug_luma(px);
            unsigned char* o = dst + (size_t)p * 3;
            o[0] = aug_blend(l, px[0], f); o[1] = aug_blend(l, px[1], f); o[2] = aug_blend(l, px[2], f);
        }
    } else {                                                                                 // every table operator
        for (int p = p0 + tid; p < p1; p += blockDim.x) {
            const int y = p / ow, x = p - y * ow;
            const unsigned char* px = src + (size_t)y * stride + (size_t)x * 3;
            unsigned char* o = dst + (size_t)p * 3;
            o[0] = lut[px[0]]; o[1] = lut[256 + px[1]]; o[2] = lut[512 + px[2]];
        }
    }
}

}  // namespace pq
