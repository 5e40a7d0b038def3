"""NumPy restatement (test infrastructure) of Pillow's `Image.filter(ImageFilter.GaussianBlur(radius))` on RGB uint8 images, the
GaussianBlur operator of the reference's training transform (strhub/data/augment.py:45-49).  It never calls the library.  Pinned against
Pillow's own outputs in tests/golden/augment_blur_pillow.npz (tools/make_augment_blur_golden.py).

Published algorithm, restated (Pillow's BoxBlur.c): a Gaussian of radius R is three box blurs of a fractional radius fr along x, then three
along y.  In SINGLE precision, with passes = 3:
    sigma2 = R * R / 3;  L = sqrt(12 sigma2 + 1);  l = floor((L - 1) / 2)
    a = (2 l + 1) (l (l + 1) - 3 sigma2) / (6 (sigma2 - (l + 1) (l + 1)));  fr = l + a
One box pass has an integer radius r = int(fr) and two 8.24 fixed-point weights, ww = uint32(float32(2^24) / (2 fr + 1)) for the 2 r + 1
inner samples and fw = (2^24 - (2 r + 1) ww) // 2 for the two samples at distance r + 1:
    out[x] = (ww * sum(in[clamp(x + i)], i = -r .. r) + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24
in 32-bit unsigned arithmetic, rounded to uint8 after EVERY pass, indices clamped to the line's ends in every pass.  Radius 0 is a copy.
`BLUR_SIZES` and `BLUR_RADII` are the cases the fixtures and the tests share; inputs are `make_input` of tests/augment_reference.py.
"""
import numpy as np

from augment_reference import apply_op

BLUR_SIZES = [(1, 1), (2, 3), (3, 2), (1, 40), (40, 1), (9, 11), (17, 53), (32, 100)]        # (height, width)
BLUR_RADII = [0, 1, 1.5, 2, 3, 4]
PASSES = 3


def blur_key(h, w, radius):
    return f'{h}x{w}_GaussianBlur_{radius}'


def box_radius(radius) -> np.float32:
    """Pillow's _gaussian_blur_radius(radius, 3): the fractional box radius, computed in C floats."""
    f = np.float32
    radius = f(radius)
    sigma2 = f(radius * radius / f(PASSES))
    big = f(np.sqrt(f(f(12.0) * sigma2 + f(1.0))))
    l = f(np.floor(f((big - f(1.0)) / f(2.0))))
    a = f(f(f(2.0) * l + f(1.0)) * f(f(l * f(l + f(1.0))) - f(f(3.0) * sigma2)))
    a = f(a / f(f(6.0) * f(sigma2 - f(f(l + f(1.0)) * f(l + f(1.0))))))
    return f(l + a)


def box_weights(radius):
    """(r, ww, fw) of one box pass for a Gaussian radius."""
    fr = box_radius(radius)
    r = int(fr)
    ww = int(np.uint32(np.float32(1 << 24) / np.float32(fr * np.float32(2.0) + np.float32(1.0))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_pass(img: np.ndarray, r: int, ww: int, fw: int) -> np.ndarray:
    """One box pass along axis 1 of uint8 [h, w, c]."""
    w = img.shape[1]
    src = img.astype(np.uint64)
    x = np.arange(w)

    def at(i):
        return src[:, np.clip(x + i, 0, w - 1)]
    acc = sum(at(i) for i in range(-r, r + 1))
    bulk = (acc * np.uint64(ww) + (at(-r - 1) + at(r + 1)) * np.uint64(fw)) & np.uint64(0xFFFFFFFF)      # 32-bit unsigned
    return (((bulk + np.uint64(1 << 23)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.uint8)


def gaussian_blur(img: np.ndarray, radius) -> np.ndarray:
    """Image.filter(ImageFilter.GaussianBlur(radius)) on uint8 [h, w, 3]."""
    if radius == 0:
        return img.copy()
    r, ww, fw = box_weights(radius)
    out = img
    for _ in range(PASSES):
        out = box_pass(out, r, ww, fw)
    out = out.transpose(1, 0, 2)
    for _ in range(PASSES):
        out = box_pass(out, r, ww, fw)
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def apply_op_with_blur(img: np.ndarray, name: str, *args) -> np.ndarray:
    """`apply_op` of tests/augment_reference.py, and GaussianBlur / PoissonNoise from the two new restatements."""
    if name == 'GaussianBlur':
        return gaussian_blur(img, args[0])
    if name == 'PoissonNoise':
        from augment_noise_reference import poisson_noise
        return poisson_noise(img, args[0], args[1])
    return apply_op(img, name, *args)


def apply_chain_with_blur(img: np.ndarray, chain) -> np.ndarray:
    """The composed reference: `apply_chain` of tests/augment_reference.py around the new restatements."""
    for op in chain:
        img = apply_op_with_blur(img, op[0], *op[1:])
    return img
