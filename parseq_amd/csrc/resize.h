// Row N2 of SURVEY.md section 8f: the resize step of the reference's input transform on the device.
//
// The reference resizes PIL images with T.Resize(img_size, BICUBIC) (strhub/data/module.py:77; read.py:41-43), i.e.
// Pillow's ImagingResample for 8-bit images (third-party, not vendored; restated in oracle/resize_oracle.py and pinned
// against Pillow's own outputs in tests/golden/resize_pillow.npz).  Bit-exactness needs the same arithmetic:
//   * tap weights in IEEE double WITHOUT fused multiply-add (hipcc contracts a * b + c by default, Pillow's x86-64 build does
//     not: AUG_NO_CONTRACT and the plain-operator macros below), normalised, then 22-bit fixed point, round half away from zero;
//   * horizontal pass first, its result clipped and stored as uint8, then the vertical pass; a pass whose size does not
//     change is skipped;  pixel = clip8((2^21 + sum in * k) >> 22) in 32-bit integers.
// One workgroup per image: the two weight tables are built in LDS (one thread per output column / row), then each thread
// produces output pixels by evaluating, for every vertical tap, the horizontal sum it needs (no intermediate image: the
// crops are small and the taps are few, so recomputing the horizontal pass per output row is cheaper than a round trip).
// The body is written once (resize_bicubic_body) over the CANVAS it reads: an image itself, or an image seen through a rotation.
#pragma once
#include "common.h"

// Exact floating-point arithmetic of the whole input path (this header, augment.h, rectify.h, rectify_mesh.h): Pillow rounds after
// every operation.  The *_rn intrinsics do not give that — hipcc defines __dmul_rn(a, b) as a * b, carrying the `contract` flag, and
// fuses it with a following add once inlined — so every function that does such arithmetic opens with AUG_NO_CONTRACT and writes its
// operations with these plain-operator macros: the pragma reaches the operations written in the function itself, not those of a callee.
// The division is the correctly rounded one (no fast-math in this build).
#define AUG_NO_CONTRACT _Pragma("clang fp contract(off)")
#define AUG_MUL(a, b) ((a) * (b))
#define AUG_ADD(a, b) ((a) + (b))
#define AUG_DIV(a, b) ((a) / (b))

namespace pq {

// RGB, HWC, uint8 (mirrors parseq_image_desc).  As the canvas of a resize it is itself: no pixel of it is black.
struct ImageDesc {
    const unsigned char* data; int height, width; long long row_stride;
    static constexpr bool has_black = false;
    __device__ int canvas_height() const { return height; }
    __device__ int canvas_width() const { return width; }
    __device__ const unsigned char* at(int x, int y) const { return data + (size_t)y * row_stride + (size_t)x * 3; }
};

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ double rs_bicubic(double x) {
    AUG_NO_CONTRACT
    const double a = -0.5;
    x = fabs(x);
    if (x < 1.0) return AUG_ADD(AUG_MUL(AUG_MUL(AUG_ADD(AUG_MUL(a + 2.0, x), -(a + 3.0)), x), x), 1.0);   // ((a+2)x - (a+3)) x x + 1
    if (x < 2.0) return AUG_MUL(AUG_ADD(AUG_MUL(AUG_ADD(AUG_MUL(AUG_ADD(x, -5.0), x), 8.0), x), -4.0), a);   // (((x-5)x + 8)x - 4) a
    return 0.0;
}

// weights of output index xx of one pass into kk[0 .. n), returns (first tap, n)
__device__ __forceinline__ void rs_coeffs(int in_size, int out_size, int xx, int* kk, int* first, int* count) {
    AUG_NO_CONTRACT
    const double scale = AUG_DIV((double)in_size, (double)out_size);
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = AUG_MUL(2.0, filterscale);
    const double ss = AUG_DIV(1.0, filterscale);
    const double center = AUG_MUL(AUG_ADD((double)xx, 0.5), scale);
    int xmin = (int)(AUG_ADD(AUG_ADD(center, -support), 0.5));
    if (xmin < 0) xmin = 0;
    int xmax = (int)(AUG_ADD(AUG_ADD(center, support), 0.5));
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww = AUG_ADD(ww, rs_bicubic(AUG_MUL(AUG_ADD(AUG_ADD((double)(x + xmin), -center), 0.5), ss)));
    for (int x = 0; x < xmax; ++x) {
        double w = rs_bicubic(AUG_MUL(AUG_ADD(AUG_ADD((double)(x + xmin), -center), 0.5), ss));
        if (ww != 0.0) w = AUG_DIV(w, ww);
        const double f = AUG_MUL(w, (double)(1 << RS_PRECISION_BITS));
        kk[x] = w < 0.0 ? (int)(AUG_ADD(-0.5, f)) : (int)(AUG_ADD(0.5, f));
    }
    *first = xmin; *count = xmax;
}

__device__ __forceinline__ int rs_clip8(int v) {
    v >>= RS_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The dynamic LDS of a resize launch, in ints: the weight tables kh [out_w][ksh] and kv [out_h][ksv] (ksh / ksv: the row pitch, the most
// taps over the batch) and the (first tap, count) pairs bh [out_w][2] and bv [out_h][2].  The kernels' pointers (I = int: a launch the host
// admitted fits) and the host's byte count (I = size_t: sizeof(int) * end, before it is known to fit) are this one map.
template <class I> struct ResizeLds { I kh, kv, bh, bv, end; };
template <class I> __host__ __device__ inline ResizeLds<I> resize_lds(int out_h, int out_w, int ksh, int ksv) {
    ResizeLds<I> m;
    m.kh = 0; m.kv = m.kh + (I)out_w * ksh; m.bh = m.kv + (I)out_h * ksv; m.bv = m.bh + 2 * (I)out_w; m.end = m.bv + 2 * (I)out_h;
    return m;
}

// Workgroup blockIdx.x resizes the canvas `cv` to its planes of out [gridDim.x][3][out_h][out_w].  A canvas has a size (canvas_height, canvas_width), at(x, y) =
// the three bytes of its pixel (x, y), or nullptr where it is black, and has_black = whether at() can ever say so.
template <class Canvas>
__device__ __forceinline__ void resize_bicubic_body(const Canvas& cv, int out_h, int out_w, int ksh, int ksv, unsigned char* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_rs[];
    const ResizeLds<int> m = resize_lds<int>(out_h, out_w, ksh, ksv);
    int* kh = reinterpret_cast<int*>(smem_rs) + m.kh;
    int* kv = reinterpret_cast<int*>(smem_rs) + m.kv;
    int* bh = reinterpret_cast<int*>(smem_rs) + m.bh;
    int* bv = reinterpret_cast<int*>(smem_rs) + m.bv;
    const int H = cv.canvas_height(), W = cv.canvas_width();
    const bool pass_h = W != out_w, pass_v = H != out_h;
    for (int i = threadIdx.x; i < out_w + out_h; i += blockDim.x) {
        if (i < out_w) { if (pass_h) rs_coeffs(W, out_w, i, kh + i * ksh, bh + 2 * i, bh + 2 * i + 1); }
        else { const int y = i - out_w; if (pass_v) rs_coeffs(H, out_h, y, kv + y * ksv, bv + 2 * y, bv + 2 * y + 1); }
    }
    __syncthreads();
    const int half = 1 << (RS_PRECISION_BITS - 1);
    unsigned char* dst = out + (size_t)blockIdx.x * 3 * out_h * out_w;
    for (int p = threadIdx.x; p < out_h * out_w; p += blockDim.x) {
        const int yy = p / out_w, xx = p - yy * out_w;
        const int x0 = pass_h ? bh[2 * xx] : xx, nx = pass_h ? bh[2 * xx + 1] : 1;
        const int y0 = pass_v ? bv[2 * yy] : yy, ny = pass_v ? bv[2 * yy + 1] : 1;
        int acc[3] = {half, half, half};
        for (int iy = 0; iy < ny; ++iy) {
            int t[3];
            if (pass_h) {
                int s0 = half, s1 = half, s2 = half;
                const int* k = kh + xx * ksh;
                for (int ix = 0; ix < nx; ++ix) {
                    const unsigned char* src = cv.at(x0 + ix, y0 + iy);
                    if (!Canvas::has_black || src) { const int w = k[ix]; s0 += (int)src[0] * w; s1 += (int)src[1] * w; s2 += (int)src[2] * w; }
                }
                t[0] = rs_clip8(s0); t[1] = rs_clip8(s1); t[2] = rs_clip8(s2);
            } else {
                const unsigned char* src = cv.at(x0, y0 + iy);
                const bool lit = !Canvas::has_black || src;
                t[0] = lit ? src[0] : 0; t[1] = lit ? src[1] : 0; t[2] = lit ? src[2] : 0;
            }
            if (pass_v) {
                const int w = kv[yy * ksv + iy];
                acc[0] += t[0] * w; acc[1] += t[1] * w; acc[2] += t[2] * w;
            } else {
                acc[0] = t[0]; acc[1] = t[1]; acc[2] = t[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[((size_t)c * out_h + yy) * out_w + xx] = (unsigned char)(pass_v ? rs_clip8(acc[c]) : acc[c]);
    }
}

// out: uint8 [B][3][out_h][out_w]
static __global__ __launch_bounds__(256)
void resize_bicubic_kernel(const ImageDesc* __restrict__ images, int out_h, int out_w, int ksh, int ksv,
                           unsigned char* __restrict__ out) {
    const ImageDesc im = images[blockIdx.x];
    resize_bicubic_body(im, out_h, out_w, ksh, ksv, out);
}

// -------------------------------------------------------------------------------------------------------------------
// Rotation ahead of the resize: the first step of the reference's evaluation transform, img.rotate(rotation, expand=True)
// (strhub/data/module.py:72-73), i.e. Pillow's Image.rotate with nearest resampling and black fill (restated in
// tests/rotate_reference.py, pinned against Pillow's outputs in tests/golden/rotate_pillow.npz).  A rotated image is never
// stored: it is a MAP from a pixel of the rot_height x rot_width canvas to a source pixel or to black.  Multiples of 90 degrees
// are exact flips / transposes; any other angle is Pillow's 16.16 fixed-point affine map, whose six integers the host derives
// with Pillow's own float64 expressions (parseq_amd/preprocess.py rotation_map) — the device does 32-bit integer arithmetic
// only, so the result is exact by construction.  The sums wrap modulo 2^32 exactly as Pillow's running `xx += a0` does; with
// every side <= ROT_MAX_SIDE the final value fits 32 bits (|source coordinate| < 20 000 < 32 768).
// rotate_resize_bicubic_kernel below is resize_bicubic_body over that canvas, every tap fetched through the map: one gather per
// tap, no rotated copy in memory.  Thread-to-pixel mapping: as over an unrotated image (consecutive lanes =
// consecutive output columns, so the stores stay coalesced).  Under a quarter turn consecutive lanes then read down a source
// COLUMN, one cache line per lane; a crop is tens of KB and one workgroup owns it, so those lines are fetched from memory once
// and every later tap of every lane hits them in the CU's vector cache / L2 (cost measured in profiles/rotate_resize.md).
// -------------------------------------------------------------------------------------------------------------------
enum { ROT_NONE = 0, ROT_90 = 1, ROT_180 = 2, ROT_270 = 3, ROT_AFFINE = 4 };
constexpr int ROT_MAX_SIDE = 16384;

struct RotatedImageDesc;
__device__ __forceinline__ const unsigned char* rot_source(const RotatedImageDesc& im, int x, int y);

// mirrors parseq_rotated_image_desc.  As the canvas of a resize it is the rotated image: rot_height x rot_width, read through rot_source.
struct RotatedImageDesc {
    const unsigned char* data; int height, width; long long row_stride;
    int mode, rot_height, rot_width;
    int a[6];
    static constexpr bool has_black = true;
    __device__ int canvas_height() const { return rot_height; }
    __device__ int canvas_width() const { return rot_width; }
    __device__ const unsigned char* at(int x, int y) const { return rot_source(*this, x, y); }
};

// source pixel of pixel (x, y) of the rotated canvas, or nullptr where Pillow fills black.  The range test also covers a
// descriptor whose rotated size does not belong to its mode: nothing outside the source is ever read.
__device__ __forceinline__ const unsigned char* rot_source(const RotatedImageDesc& im, int x, int y) {
    int sx, sy;
    switch (im.mode) {
        case ROT_NONE: sx = x; sy = y; break;
        case ROT_90: sx = im.width - 1 - y; sy = x; break;                       // transpose, then rows reversed
        case ROT_180: sx = im.width - 1 - x; sy = im.height - 1 - y; break;
        case ROT_270: sx = y; sy = im.height - 1 - x; break;                     // transpose, then columns reversed
        default:
            sx = (int)((unsigned)im.a[2] + (unsigned)im.a[0] * (unsigned)x + (unsigned)im.a[1] * (unsigned)y) >> 16;
            sy = (int)((unsigned)im.a[5] + (unsigned)im.a[3] * (unsigned)x + (unsigned)im.a[4] * (unsigned)y) >> 16;
    }
    if ((unsigned)sx >= (unsigned)im.width || (unsigned)sy >= (unsigned)im.height) return nullptr;
    return im.data + (size_t)sy * im.row_stride + (size_t)sx * 3;
}

// out: uint8 [rot_height][rot_width][3], the rotated image itself (parseq_op_rotate: what the kernel tests compare with Pillow)
static __global__ __launch_bounds__(256)
void rotate_kernel(const RotatedImageDesc im, unsigned char* __restrict__ out) {
    const int n = im.rot_height * im.rot_width;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int y = p / im.rot_width, x = p - y * im.rot_width;
        const unsigned char* src = rot_source(im, x, y);
        unsigned char* dst = out + (size_t)p * 3;
        dst[0] = src ? src[0] : 0; dst[1] = src ? src[1] : 0; dst[2] = src ? src[2] : 0;
    }
}

// the resize over the rotated canvas of every image.  out: uint8 [B][3][out_h][out_w].
static __global__ __launch_bounds__(256)
void rotate_resize_bicubic_kernel(const RotatedImageDesc* __restrict__ images, int out_h, int out_w, int ksh, int ksv,
                                  unsigned char* __restrict__ out) {
    const RotatedImageDesc im = images[blockIdx.x];
    resize_bicubic_body(im, out_h, out_w, ksh, ksv, out);
}

}  // namespace pq
