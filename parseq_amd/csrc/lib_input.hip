// libparseq_hip.so — the input path: resize, rotate, augment and rectify (quadrilaterals and polygons) on the device, each alone and ahead
// of the one resize.  Every rule of the path stands here once: the image and output checks, the resize plan (taps, LDS bytes, the cap)
// and its launch, the region checks and the one run of a rectification.  Every refusal comes before the first device call.
#include "lib_internal.h"
#include "rectify_mesh.h"

#include <type_traits>

static_assert(sizeof(parseq_image_desc) == sizeof(ImageDesc), "descriptor layouts must match");
static_assert(sizeof(parseq_rotated_image_desc) == sizeof(RotatedImageDesc) && offsetof(parseq_rotated_image_desc, a) == offsetof(RotatedImageDesc, a) &&
              PARSEQ_ROTATE_AFFINE == ROT_AFFINE && PARSEQ_ROTATE_MAX_SIDE == ROT_MAX_SIDE, "descriptor layouts must match");
static_assert(sizeof(parseq_augment_op) == sizeof(AugOp) && offsetof(parseq_augment_op, arg) == offsetof(AugOp, arg) &&
              sizeof(parseq_augment_desc) == sizeof(AugDesc) && offsetof(parseq_augment_desc, ops) == offsetof(AugDesc, ops) &&
              PARSEQ_AUGMENT_MAX_OPS == AUG_MAX_OPS && PARSEQ_AUG_TURN == AUG_TURN && PARSEQ_AUG_TABLE == AUG_TABLE &&
              PARSEQ_AUG_BICUBIC == AUG_BICUBIC && PARSEQ_AUG_GAUSSIAN_BLUR == AUG_GAUSSIAN_BLUR && PARSEQ_AUG_POISSON_NOISE == AUG_POISSON_NOISE &&
              sizeof(parseq_augment_op) == 16 + 256 && offsetof(parseq_augment_op, arg.blur.fw) == offsetof(AugOp, arg.blur.fw) &&
              offsetof(parseq_augment_op, arg.noise.lam) == offsetof(AugOp, arg.noise.lam), "descriptor layouts must match");
static_assert(sizeof(parseq_region_desc) == sizeof(RegionDesc) && offsetof(parseq_region_desc, coef) == offsetof(RegionDesc, coef) &&
              offsetof(parseq_region_desc, width) == offsetof(RegionDesc, width), "descriptor layouts must match");
static_assert(sizeof(parseq_mesh_strip) == sizeof(MeshStrip) && offsetof(parseq_mesh_strip, coef) == offsetof(MeshStrip, coef) &&
              sizeof(parseq_mesh_region_desc) == sizeof(MeshRegionDesc) && offsetof(parseq_mesh_region_desc, n_strips) == offsetof(MeshRegionDesc, n_strips) &&
              PARSEQ_MESH_MAX_STRIPS == MESH_MAX_STRIPS, "descriptor layouts must match");

// -------------------------------------------------------------------------------------------------------------------
// what every call shares: the image and output checks, the plan of the resize and its launch
// -------------------------------------------------------------------------------------------------------------------
// image i of a call, whatever its descriptor carries beyond these four fields
static int check_image(const parseq_image_desc& d, int i) {
    if (!d.data || d.height <= 0 || d.width <= 0 || d.row_stride < (int64_t)d.width * 3)
        return fail(PARSEQ_E_INVALID, "image %d: bad descriptor (%dx%d, row stride %lld)", i, d.height, d.width, (long long)d.row_stride);
    return 0;
}

// the output of a fused call whose other arguments have checks of their own
static int check_output(const uint8_t* out, int out_h, int out_w) {
    if (!out) return fail(PARSEQ_E_INVALID, "null out");
    if (out_h <= 0 || out_w <= 0) return fail(PARSEQ_E_INVALID, "bad shape: output %dx%d", out_h, out_w);
    return 0;
}

static int resize_taps(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

// The resize of n items to out_h x out_w: the row pitch of the two tap tables (the most taps over the items) and the LDS they take
// (resize.h ResizeLds).  size_of(i, &h, &w) = the size of item i as the resize reads it; `what` names an item in the refusal.
struct ResizePlan { int out_h, out_w, ksh, ksv; size_t lds; };

template <class SizeOf>
static int resize_plan(int n, SizeOf size_of, int out_h, int out_w, const char* what, ResizePlan* z) {
    z->out_h = out_h; z->out_w = out_w; z->ksh = z->ksv = 1;
    for (int i = 0; i < n; ++i) {
        int h, w;
        size_of(i, &h, &w);
        z->ksh = std::max(z->ksh, resize_taps(w, out_w));
        z->ksv = std::max(z->ksv, resize_taps(h, out_h));
    }
    z->lds = sizeof(int) * resize_lds<size_t>(out_h, out_w, z->ksh, z->ksv).end;
    if (z->lds > 150 * 1024) return fail(PARSEQ_E_INVALID, "%s is too large for the on-chip weight tables (%zu bytes of LDS needed)", what, z->lds);
    return 0;
}

// one of the two resize kernels over the n descriptors at `descs` (device memory): one workgroup per item
template <class Desc>
static int resize_launch(void (*kernel)(const Desc*, int, int, int, int, unsigned char*), const void* descs, int n, const ResizePlan& z, uint8_t* out,
                         hipStream_t s) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)z.lds));     // size varies per call
    hipLaunchKernelGGL(kernel, dim3(n), dim3(256), z.lds, s, static_cast<const Desc*>(descs), z.out_h, z.out_w, z.ksh, z.ksv, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// -------------------------------------------------------------------------------------------------------------------
// resize, and rotate + resize: the first two steps of the reference's evaluation transform (strhub/data/module.py:72-77) in one launch
// -------------------------------------------------------------------------------------------------------------------
extern "C" size_t parseq_resize_workspace_bytes(int batch) { return batch > 0 ? (size_t)batch * sizeof(ImageDesc) : 0; }

extern "C" int parseq_resize_bicubic(const parseq_image_desc* images, int batch, int out_h, int out_w, uint8_t* out, void* workspace,
                                     void* stream) {
    if (!images || !out || !workspace) return fail(PARSEQ_E_INVALID, "null images / out / workspace");
    if (batch <= 0 || out_h <= 0 || out_w <= 0) return fail(PARSEQ_E_INVALID, "bad shape: batch %d, output %dx%d", batch, out_h, out_w);
    for (int i = 0; i < batch; ++i) CHK(check_image(images[i], i));
    ResizePlan z;
    CHK(resize_plan(batch, [&](int i, int* h, int* w) { *h = images[i].height; *w = images[i].width; }, out_h, out_w, "an image", &z));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(workspace, images, (size_t)batch * sizeof(ImageDesc), hipMemcpyHostToDevice, s));
    return resize_launch(resize_bicubic_kernel, workspace, batch, z, out, s);
}

static int check_rotated(const parseq_rotated_image_desc& d, int i) {
    CHK(check_image({d.data, d.height, d.width, d.row_stride}, i));
    const bool turned = d.mode == PARSEQ_ROTATE_90 || d.mode == PARSEQ_ROTATE_270;
    switch (d.mode) {
        case PARSEQ_ROTATE_NONE: case PARSEQ_ROTATE_90: case PARSEQ_ROTATE_180: case PARSEQ_ROTATE_270:
            if (d.rot_height != (turned ? d.width : d.height) || d.rot_width != (turned ? d.height : d.width))
                return fail(PARSEQ_E_INVALID, "image %d: mode %d turns %dx%d into %dx%d, not %dx%d", i, d.mode, d.height, d.width,
                            turned ? d.width : d.height, turned ? d.height : d.width, d.rot_height, d.rot_width);
            break;
        case PARSEQ_ROTATE_AFFINE:
            if (d.rot_height <= 0 || d.rot_width <= 0) return fail(PARSEQ_E_INVALID, "image %d: rotated size %dx%d", i, d.rot_height, d.rot_width);
            break;
        default: return fail(PARSEQ_E_INVALID, "image %d: unknown rotation mode %d", i, d.mode);
    }
    if (std::max(std::max(d.height, d.width), std::max(d.rot_height, d.rot_width)) > PARSEQ_ROTATE_MAX_SIDE)
        return fail(PARSEQ_E_INVALID, "image %d: %dx%d rotated to %dx%d, a side is above %d (the map is 32-bit fixed point)", i, d.height, d.width,
                    d.rot_height, d.rot_width, PARSEQ_ROTATE_MAX_SIDE);
    return 0;
}

extern "C" size_t parseq_rotate_resize_workspace_bytes(int batch) { return batch > 0 ? (size_t)batch * sizeof(RotatedImageDesc) : 0; }

extern "C" int parseq_rotate_resize_bicubic(const parseq_rotated_image_desc* images, int batch, int out_h, int out_w, uint8_t* out,
                                            void* workspace, void* stream) {
    if (!images || !out || !workspace) return fail(PARSEQ_E_INVALID, "null images / out / workspace");
    if (batch <= 0 || out_h <= 0 || out_w <= 0) return fail(PARSEQ_E_INVALID, "bad shape: batch %d, output %dx%d", batch, out_h, out_w);
    for (int i = 0; i < batch; ++i) CHK(check_rotated(images[i], i));
    ResizePlan z;
    CHK(resize_plan(batch, [&](int i, int* h, int* w) { *h = images[i].rot_height; *w = images[i].rot_width; }, out_h, out_w, "a rotated image", &z));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(workspace, images, (size_t)batch * sizeof(RotatedImageDesc), hipMemcpyHostToDevice, s));
    return resize_launch(rotate_resize_bicubic_kernel, workspace, batch, z, out, s);
}

extern "C" int parseq_op_rotate(const parseq_rotated_image_desc* image, uint8_t* out, void* stream) {
    if (!image || !out) return fail(PARSEQ_E_INVALID, "null image / out");
    CHK(check_rotated(*image, 0));
    RotatedImageDesc im;
    memcpy(&im, image, sizeof(im));
    const long long pixels = (long long)im.rot_height * im.rot_width;
    hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)std::min<long long>((pixels + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, im, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// -------------------------------------------------------------------------------------------------------------------
// training augmentation (augment.h): chains of Pillow-exact RandAugment operators, then the resize
// -------------------------------------------------------------------------------------------------------------------
static bool aug_side_ok(int v) { return v >= 1 && v <= PARSEQ_ROTATE_MAX_SIDE; }

static int check_augment(const parseq_augment_desc& d, int i) {
    CHK(check_image({d.data, d.height, d.width, d.row_stride}, i));
    if (!aug_side_ok(d.height) || !aug_side_ok(d.width))
        return fail(PARSEQ_E_INVALID, "image %d: %dx%d, a side is above %d", i, d.height, d.width, PARSEQ_ROTATE_MAX_SIDE);
    if (d.num_ops < 0 || d.num_ops > PARSEQ_AUGMENT_MAX_OPS)
        return fail(PARSEQ_E_INVALID, "image %d: %d operators, a chain holds at most %d", i, d.num_ops, PARSEQ_AUGMENT_MAX_OPS);
    int h = d.height, w = d.width;
    for (int k = 0; k < d.num_ops; ++k) {
        const parseq_augment_op& op = d.ops[k];
        if (!aug_side_ok(op.out_height) || !aug_side_ok(op.out_width))
            return fail(PARSEQ_E_INVALID, "image %d, operator %d: output of %dx%d, each side must be in 1 .. %d", i, k, op.out_height, op.out_width,
                        PARSEQ_ROTATE_MAX_SIDE);
        const bool same = op.out_height == h && op.out_width == w;
        switch (op.op) {
            case PARSEQ_AUG_TABLE: case PARSEQ_AUG_AUTOCONTRAST: case PARSEQ_AUG_EQUALIZE: break;
            case PARSEQ_AUG_CONTRAST: case PARSEQ_AUG_COLOR:
                if (!(std::isfinite(op.arg.factor) && op.arg.factor >= 0.1f))
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: factor %g is out of range (finite, >= 0.1)", i, k, (double)op.arg.factor);
                break;
            case PARSEQ_AUG_AFFINE:
                if (op.mode != PARSEQ_AUG_BILINEAR && op.mode != PARSEQ_AUG_BICUBIC)
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: resample %d is out of range (2 bilinear, 3 bicubic)", i, k, op.mode);
                for (int t = 0; t < 6; ++t)
                    if (!std::isfinite(op.arg.coef[t]))
                        return fail(PARSEQ_E_INVALID, "image %d, operator %d: coefficient %d is out of range (not finite)", i, k, t);
                break;
            case PARSEQ_AUG_TURN: {
                if (op.mode != PARSEQ_ROTATE_90 && op.mode != PARSEQ_ROTATE_180 && op.mode != PARSEQ_ROTATE_270)
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: turn %d is out of range (1, 2 or 3 quarter turns)", i, k, op.mode);
                const bool swap = op.mode != PARSEQ_ROTATE_180;
                if (op.out_height != (swap ? w : h) || op.out_width != (swap ? h : w))
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: turn %d makes %dx%d of %dx%d, not %dx%d", i, k, op.mode, swap ? w : h, swap ? h : w,
                                h, w, op.out_height, op.out_width);
                break;
            }
            case PARSEQ_AUG_GAUSSIAN_BLUR: {
                if (op.arg.blur.r < 0 || op.arg.blur.r > AUG_BLUR_MAX_R)
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: blur radius r %d is out of range (0 .. %d)", i, k, op.arg.blur.r, AUG_BLUR_MAX_R);
                const unsigned long long sum = (2ull * (unsigned)op.arg.blur.r + 1) * op.arg.blur.ww + 2ull * op.arg.blur.fw;
                if (sum > (1ull << 24))
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: blur weights ww %u, fw %u are out of range ((2 r + 1) ww + 2 fw = %llu, above 2^24)",
                                i, k, op.arg.blur.ww, op.arg.blur.fw, sum);
                break;
            }
            case PARSEQ_AUG_POISSON_NOISE:
                if (op.arg.noise.lam < 1 || op.arg.noise.lam > AUG_NOISE_MAX_LAM)
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: noise lam %d is out of range (1 .. %d)", i, k, op.arg.noise.lam, AUG_NOISE_MAX_LAM);
                if (!(std::isfinite(op.arg.noise.p0) && op.arg.noise.p0 > 0.0 && op.arg.noise.p0 < 1.0))
                    return fail(PARSEQ_E_INVALID, "image %d, operator %d: noise p0 %g is out of range (exp(-lam): finite, in (0, 1))", i, k, op.arg.noise.p0);
                break;
            default: return fail(PARSEQ_E_INVALID, "image %d, operator %d: unknown operator %d", i, k, op.op);
        }
        if (op.op != PARSEQ_AUG_AFFINE && op.op != PARSEQ_AUG_TURN && !same)
            return fail(PARSEQ_E_INVALID, "image %d, operator %d: operator %d keeps the size, %dx%d stated for %dx%d", i, k, op.op, op.out_height,
                        op.out_width, h, w);
        h = op.out_height; w = op.out_width;
    }
    return 0;
}

struct AugLayout { size_t descs, offsets, finals, regions, total; };

static size_t aug_align(size_t v) { return (v + 255) & ~(size_t)255; }

static AugLayout aug_layout(const parseq_augment_desc* descs, int batch) {
    AugLayout l;
    l.descs = 0;
    l.offsets = aug_align((size_t)batch * sizeof(AugDesc));
    l.finals = l.offsets + aug_align((size_t)batch * sizeof(size_t));
    l.regions = l.finals + aug_align((size_t)batch * sizeof(ImageDesc));
    l.total = l.regions;
    for (int i = 0; i < batch; ++i) l.total += 2 * aug_region_bytes(descs[i]);
    return l;
}

extern "C" size_t parseq_augment_workspace_bytes(const parseq_augment_desc* descs, int batch) {
    if (!descs || batch <= 0) { fail(PARSEQ_E_INVALID, "null descriptors / batch %d", batch); return 0; }
    for (int i = 0; i < batch; ++i)
        if (check_augment(descs[i], i)) return 0;
    return aug_layout(descs, batch).total;
}

// validates, copies the descriptors, plans the regions and runs every stage on `s`
static int augment_run(const parseq_augment_desc* descs, int batch, void* workspace, size_t workspace_bytes, hipStream_t s, AugLayout* layout) {
    if (!descs || !workspace) return fail(PARSEQ_E_INVALID, "null descriptors / workspace");
    if (batch <= 0) return fail(PARSEQ_E_INVALID, "bad shape: batch %d", batch);
    for (int i = 0; i < batch; ++i) CHK(check_augment(descs[i], i));
    const AugLayout l = aug_layout(descs, batch);
    if (workspace_bytes < l.total)
        return fail(PARSEQ_E_INVALID, "workspace of %zu bytes, %zu needed (parseq_augment_workspace_bytes)", workspace_bytes, l.total);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const AugDesc* dd = reinterpret_cast<const AugDesc*>(ws + l.descs);
    size_t* offsets = reinterpret_cast<size_t*>(ws + l.offsets);
    HIPCHK(hipMemcpyAsync(ws + l.descs, descs, (size_t)batch * sizeof(AugDesc), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(augment_plan_kernel, dim3(1), dim3(256), 0, s, dd, batch, ws + l.regions, offsets, reinterpret_cast<ImageDesc*>(ws + l.finals));
    HIPCHK(hipGetLastError());
    for (int k = 0; k < PARSEQ_AUGMENT_MAX_OPS; ++k) {
        int tiles = 0;
        for (int i = 0; i < batch; ++i)
            if (descs[i].num_ops > k) tiles = std::max(tiles, aug_tiles((long long)descs[i].ops[k].out_height * descs[i].ops[k].out_width));
        if (!tiles) break;                                   // chains are dense: no image has an operator k + 1 without an operator k
        hipLaunchKernelGGL(augment_stage_kernel, dim3(batch, tiles), dim3(256), 0, s, dd, offsets, ws + l.regions, k);
        HIPCHK(hipGetLastError());
    }
    *layout = l;
    return 0;
}

extern "C" int parseq_augment_resize_bicubic(const parseq_augment_desc* descs, int batch, int out_h, int out_w, uint8_t* out, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    CHK(check_output(out, out_h, out_w));
    if (!descs || batch <= 0) return fail(PARSEQ_E_INVALID, "null descriptors / batch %d", batch);
    for (int i = 0; i < batch; ++i) CHK(check_augment(descs[i], i));
    ResizePlan z;
    CHK(resize_plan(batch, [&](int i, int* h, int* w) {
        const parseq_augment_desc& d = descs[i];
        *h = d.num_ops ? d.ops[d.num_ops - 1].out_height : d.height; *w = d.num_ops ? d.ops[d.num_ops - 1].out_width : d.width;
    }, out_h, out_w, "an augmented image", &z));
    hipStream_t s = (hipStream_t)stream;
    AugLayout l;
    CHK(augment_run(descs, batch, workspace, workspace_bytes, s, &l));
    return resize_launch(resize_bicubic_kernel, static_cast<unsigned char*>(workspace) + l.finals, batch, z, out, s);
}

extern "C" int parseq_op_augment(const parseq_augment_desc* desc, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !out) return fail(PARSEQ_E_INVALID, "null descriptor / out");
    hipStream_t s = (hipStream_t)stream;
    AugLayout l;
    CHK(augment_run(desc, 1, workspace, workspace_bytes, s, &l));
    const int n = desc->num_ops;
    const int h = n ? desc->ops[n - 1].out_height : desc->height, w = n ? desc->ops[n - 1].out_width : desc->width;
    const unsigned char* last = n ? static_cast<unsigned char*>(workspace) + l.regions + (size_t)((n - 1) & 1) * aug_region_bytes(*desc) : desc->data;
    HIPCHK(hipMemcpy2DAsync(out, (size_t)w * 3, last, n ? (size_t)w * 3 : (size_t)desc->row_stride, (size_t)w * 3, (size_t)h, hipMemcpyDeviceToDevice, s));
    return 0;
}

// -------------------------------------------------------------------------------------------------------------------
// rectification of regions, alone and ahead of the resize: quadrilaterals (rectify.h, Region = parseq_region_desc) and polygons as strips
// (rectify_mesh.h, Region = parseq_mesh_region_desc): one plan, one workspace, one run; the polygons bring one more table
// -------------------------------------------------------------------------------------------------------------------
// `strips`: the strip table of polygon regions, empty for quadrilaterals
struct RectLayout { size_t regions, strips, images, tiles, dst, finals, outs, slots, total; long long n_tiles; };

template <class Region>
static int check_region_size(const Region& r, int i) {
    if (!aug_side_ok(r.height) || !aug_side_ok(r.width))
        return fail(PARSEQ_E_INVALID, "region %d: size %dx%d, each side must be in 1 .. %d", i, r.height, r.width, PARSEQ_ROTATE_MAX_SIDE);
    return 0;
}

// what every kind of region has: the image it reads and its size
template <class Region>
static int check_region_common(const Region& r, int i, int n_images) {
    if (r.image < 0 || r.image >= n_images) return fail(PARSEQ_E_INVALID, "region %d: image index %d is outside 0 .. %d", i, r.image, n_images - 1);
    return check_region_size(r, i);
}

// sizes only: what the *_workspace_bytes functions can know
template <class Region>
static RectLayout rect_layout(const Region* regions, int n, int n_images, int n_strips = 0) {
    RectLayout l;
    l.regions = 0;
    l.strips = l.regions + aug_align((size_t)n * sizeof(Region));
    l.images = l.strips + aug_align((size_t)n_strips * sizeof(MeshStrip));
    l.tiles = l.images + aug_align((size_t)n_images * sizeof(ImageDesc));
    l.dst = l.tiles + aug_align((size_t)(n + 1) * sizeof(int));
    l.finals = l.dst + aug_align((size_t)n * sizeof(unsigned char*));
    l.outs = l.finals + aug_align((size_t)n * sizeof(ImageDesc));
    l.slots = l.outs + aug_align((size_t)n * sizeof(unsigned char*));
    l.total = l.slots;
    l.n_tiles = 0;
    for (int i = 0; i < n; ++i) {
        l.total += rect_slot_bytes(regions[i].height, regions[i].width);
        l.n_tiles += rect_tiles(regions[i].height, regions[i].width);
    }
    return l;
}

// the source images of a rectification
static int check_rect_images(const parseq_image_desc* images, int n_images) {
    for (int i = 0; i < n_images; ++i) {
        const parseq_image_desc& d = images[i];
        CHK(check_image(d, i));
        if (d.row_stride > INT32_MAX / d.height)
            return fail(PARSEQ_E_INVALID, "image %d: %d rows of %lld bytes do not fit 31 bits", i, d.height, (long long)d.row_stride);
    }
    return 0;
}

// the buffers of a caller who takes the rectified regions themselves
static int check_outs(uint8_t* const* outs, int n) {
    if (!outs) return fail(PARSEQ_E_INVALID, "null outs");
    for (int i = 0; i < n; ++i)
        if (!outs[i]) return fail(PARSEQ_E_INVALID, "region %d: null output", i);
    return 0;
}

// Copies the regions, the strip table (if any), the images and `outs` (if any) into the workspace, plans and rectifies on `s`: ONE launch
// for all regions after the plan, by the kernel that belongs to Region.  The descriptors have passed check_rectify / check_mesh.
template <class Region>
static int rect_run(const parseq_image_desc* images, int n_images, const Region* regions, int n, const parseq_mesh_strip* strips, int n_strips,
                    uint8_t* const* outs, void* workspace, size_t workspace_bytes, hipStream_t s, RectLayout* layout) {
    constexpr bool mesh = std::is_same<Region, parseq_mesh_region_desc>::value;
    using DevRegion = typename std::conditional<mesh, MeshRegionDesc, RegionDesc>::type;
    if (!workspace) return fail(PARSEQ_E_INVALID, "null workspace");
    const RectLayout l = rect_layout(regions, n, n_images, n_strips);
    if (workspace_bytes < l.total)
        return fail(PARSEQ_E_INVALID, "workspace of %zu bytes, %zu needed (%s)", workspace_bytes, l.total,
                    mesh ? "parseq_mesh_rectify_workspace_bytes" : "parseq_rectify_workspace_bytes");
    if (l.n_tiles > RECT_MAX_TILES)                      // 256 work-items each: the launch holds fewer than 2^32 of them
        return fail(PARSEQ_E_INVALID, "%lld tiles of %dx%d pixels in one call, at most %d", l.n_tiles, RECT_TILE, RECT_TILE, RECT_MAX_TILES);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const DevRegion* rr = reinterpret_cast<const DevRegion*>(ws + l.regions);
    const ImageDesc* ii = reinterpret_cast<const ImageDesc*>(ws + l.images);
    int* tile_start = reinterpret_cast<int*>(ws + l.tiles);
    unsigned char** dst = reinterpret_cast<unsigned char**>(ws + l.dst);
    unsigned char** douts = nullptr;
    HIPCHK(hipMemcpyAsync(ws + l.regions, regions, (size_t)n * sizeof(Region), hipMemcpyHostToDevice, s));
    if (mesh) HIPCHK(hipMemcpyAsync(ws + l.strips, strips, (size_t)n_strips * sizeof(MeshStrip), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ws + l.images, images, (size_t)n_images * sizeof(ImageDesc), hipMemcpyHostToDevice, s));
    if (outs) {
        douts = reinterpret_cast<unsigned char**>(ws + l.outs);
        HIPCHK(hipMemcpyAsync(douts, outs, (size_t)n * sizeof(unsigned char*), hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(rectify_plan_kernel<DevRegion>, dim3(1), dim3(256), 0, s, rr, n, douts, ws + l.slots, tile_start, dst,
                       reinterpret_cast<ImageDesc*>(ws + l.finals));
    HIPCHK(hipGetLastError());
    if constexpr (mesh)
        hipLaunchKernelGGL(mesh_rectify_kernel, dim3((unsigned)l.n_tiles), dim3(256), 0, s, ii, n_images, rr, n, reinterpret_cast<const MeshStrip*>(ws + l.strips),
                           tile_start, dst);
    else
        hipLaunchKernelGGL(rectify_kernel, dim3((unsigned)l.n_tiles), dim3(256), 0, s, ii, n_images, rr, n, tile_start, dst);
    HIPCHK(hipGetLastError());
    *layout = l;
    return 0;
}

// rect_run without `outs`, then the resize of the ImageDesc array the plan kernel wrote; the resize is planned before any device work
template <class Region>
static int rect_resize_run(const parseq_image_desc* images, int n_images, const Region* regions, int n, const parseq_mesh_strip* strips, int n_strips,
                           int out_h, int out_w, uint8_t* out, void* workspace, size_t workspace_bytes, hipStream_t s) {
    ResizePlan z;
    CHK(resize_plan(n, [&](int i, int* h, int* w) { *h = regions[i].height; *w = regions[i].width; }, out_h, out_w, "a rectified region", &z));
    RectLayout l;
    CHK(rect_run(images, n_images, regions, n, strips, n_strips, nullptr, workspace, workspace_bytes, s, &l));
    return resize_launch(resize_bicubic_kernel, static_cast<unsigned char*>(workspace) + l.finals, n, z, out, s);
}

// ---- quadrilaterals
extern "C" size_t parseq_rectify_workspace_bytes(const parseq_region_desc* regions, int n_regions, int n_images) {
    if (!regions || n_regions <= 0 || n_images <= 0) { fail(PARSEQ_E_INVALID, "null regions / %d regions / %d images", n_regions, n_images); return 0; }
    for (int i = 0; i < n_regions; ++i)
        if (check_region_size(regions[i], i)) return 0;
    return rect_layout(regions, n_regions, n_images).total;
}

static int check_rectify(const parseq_image_desc* images, int n_images, const parseq_region_desc* regions, int n) {
    if (!images || !regions) return fail(PARSEQ_E_INVALID, "null images / regions");
    if (n_images <= 0 || n <= 0) return fail(PARSEQ_E_INVALID, "bad shape: %d images, %d regions", n_images, n);
    CHK(check_rect_images(images, n_images));
    for (int i = 0; i < n; ++i) {
        const parseq_region_desc& r = regions[i];
        CHK(check_region_common(r, i, n_images));
        for (int t = 0; t < 8; ++t)
            if (!std::isfinite(r.coef[t])) return fail(PARSEQ_E_INVALID, "region %d: coefficient %d is not finite", i, t);
        const double w = r.width, h = r.height;
        const double corners[4][2] = {{0.0, 0.0}, {w, 0.0}, {w, h}, {0.0, h}};
        for (const auto& c : corners) {
            const double den = r.coef[6] * c[0] + r.coef[7] * c[1] + 1.0;
            if (!(den > 0.0))
                return fail(PARSEQ_E_INVALID, "region %d: the denominator is %g at output corner (%g, %g), it must be > 0 over the output", i, den, c[0], c[1]);
        }
    }
    return 0;
}

extern "C" int parseq_rectify(const parseq_image_desc* images, int n_images, const parseq_region_desc* regions, int n_regions, uint8_t* const* outs,
                              void* workspace, size_t workspace_bytes, void* stream) {
    CHK(check_rectify(images, n_images, regions, n_regions));
    CHK(check_outs(outs, n_regions));
    RectLayout l;
    return rect_run(images, n_images, regions, n_regions, nullptr, 0, outs, workspace, workspace_bytes, (hipStream_t)stream, &l);
}

extern "C" int parseq_rectify_resize_bicubic(const parseq_image_desc* images, int n_images, const parseq_region_desc* regions, int n_regions,
                                             int out_h, int out_w, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    CHK(check_output(out, out_h, out_w));
    CHK(check_rectify(images, n_images, regions, n_regions));
    return rect_resize_run(images, n_images, regions, n_regions, nullptr, 0, out_h, out_w, out, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- polygons
extern "C" size_t parseq_mesh_rectify_workspace_bytes(const parseq_mesh_region_desc* regions, int n_regions, const parseq_mesh_strip* strips, int n_strips,
                                                      int n_images) {
    if (!regions || !strips || n_regions <= 0 || n_strips <= 0 || n_images <= 0) {
        fail(PARSEQ_E_INVALID, "null regions / strips / %d regions / %d strips / %d images", n_regions, n_strips, n_images);
        return 0;
    }
    for (int i = 0; i < n_regions; ++i)
        if (check_region_size(regions[i], i)) return 0;
    return rect_layout(regions, n_regions, n_images, n_strips).total;
}

static int check_mesh(const parseq_image_desc* images, int n_images, const parseq_mesh_region_desc* regions, int n, const parseq_mesh_strip* strips,
                      int n_strips) {
    if (!images || !regions || !strips) return fail(PARSEQ_E_INVALID, "null images / regions / strips");
    if (n_images <= 0 || n <= 0 || n_strips <= 0) return fail(PARSEQ_E_INVALID, "bad shape: %d images, %d regions, %d strips", n_images, n, n_strips);
    CHK(check_rect_images(images, n_images));
    for (int i = 0; i < n; ++i) {
        const parseq_mesh_region_desc& r = regions[i];
        CHK(check_region_common(r, i, n_images));
        if (r.n_strips < 1 || r.n_strips > PARSEQ_MESH_MAX_STRIPS)
            return fail(PARSEQ_E_INVALID, "region %d: %d strips, a region has 1 .. %d", i, r.n_strips, PARSEQ_MESH_MAX_STRIPS);
        if (r.first_strip < 0 || r.first_strip > n_strips - r.n_strips)
            return fail(PARSEQ_E_INVALID, "region %d: strips %d .. %d are outside the strips array of %d", i, r.first_strip, r.first_strip + r.n_strips - 1, n_strips);
        int at = 0;
        for (int k = 0; k < r.n_strips; ++k) {
            const parseq_mesh_strip& s = strips[r.first_strip + k];
            if (s.x0 != at || s.x1 <= s.x0 || s.x1 > r.width)
                return fail(PARSEQ_E_INVALID, "region %d: strip %d covers columns %d .. %d where %d begins: the strips must tile 0 .. %d in order", i, k, s.x0,
                            s.x1, at, r.width);
            at = s.x1;
            for (int t = 0; t < 8; ++t)
                if (!std::isfinite(s.coef[t])) return fail(PARSEQ_E_INVALID, "region %d: strip %d: coefficient %d is not finite", i, k, t);
        }
        if (at != r.width) return fail(PARSEQ_E_INVALID, "region %d: the strips end at column %d: they must tile 0 .. %d", i, at, r.width);
    }
    return 0;
}

extern "C" int parseq_mesh_rectify(const parseq_image_desc* images, int n_images, const parseq_mesh_region_desc* regions, int n_regions,
                                   const parseq_mesh_strip* strips, int n_strips, uint8_t* const* outs, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    CHK(check_mesh(images, n_images, regions, n_regions, strips, n_strips));
    CHK(check_outs(outs, n_regions));
    RectLayout l;
    return rect_run(images, n_images, regions, n_regions, strips, n_strips, outs, workspace, workspace_bytes, (hipStream_t)stream, &l);
}

extern "C" int parseq_mesh_rectify_resize_bicubic(const parseq_image_desc* images, int n_images, const parseq_mesh_region_desc* regions, int n_regions,
                                                  const parseq_mesh_strip* strips, int n_strips, int out_h, int out_w, uint8_t* out, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
    CHK(check_output(out, out_h, out_w));
    CHK(check_mesh(images, n_images, regions, n_regions, strips, n_strips));
    return rect_resize_run(images, n_images, regions, n_regions, strips, n_strips, out_h, out_w, out, workspace, workspace_bytes, (hipStream_t)stream);
}
