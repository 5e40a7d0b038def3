"""NumPy restatement (test infrastructure) of the PoissonNoise operator of the training transform.  It never calls the library.

The reference calls imgaug's AdditivePoissonNoise(lam) (strhub/data/augment.py:66-70), which imgaug publishes as
AddElementwise(RandomSign(Poisson(lam)), per_channel=False).  imgaug is not installed here, so this is a STATED definition, not a pinned one:
per pixel one draw n = +-k, k ~ Poisson(lam), both signs equally likely; the same n is added to R, G and B; the result is clipped to 0 .. 255.

The draw (numpy integers and float64 only):
  * Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123), key = (low, high word of
    the 64-bit seed), counter = (pixel index y * width + x: low word, high word, 0, 0);
  * word 0 is the uniform u in 0 .. 2^32 - 1; bit 31 of word 1 set means n = -k;
  * k = the number of thresholds T_j <= u, j = 0 .. 126, with T_j = min(floor(C_j 2^32), 2^32 - 1), C_j = C_(j-1) + p_j,
    p_(j+1) = (p_j lam) / (j + 1), p_0 = exp(-lam), one float64 operation at a time.
The mutants at the end are what tests/test_augment_blur_noise.py shows its distribution check can tell from the definition.
"""
import math

import numpy as np

LEVELS = 127
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or integers) of 32-bit words, key: two.  Returns the four uint64 arrays of output words."""
    c = [np.asarray(v, np.uint64) & MASK for v in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                                 # 32 x 32 -> 64 bits: no wrap in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def thresholds(lam: int) -> np.ndarray:
    """uint64 [127]: T_j of the module docstring."""
    out = []
    p = c = np.float64(math.exp(-lam))
    for j in range(LEVELS):
        out.append(min(int(math.floor(c * np.float64(4294967296.0))), 2 ** 32 - 1))
        p = (p * np.float64(lam)) / np.float64(j + 1)
        c = c + p
    return np.array(out, np.uint64)


def noise_field(h: int, w: int, lam: int, seed: int, sign_word: int = 1) -> np.ndarray:
    """int64 [h, w]: the n of every pixel."""
    index = np.arange(h * w, dtype=np.uint64)
    words = philox4x32_10((index & MASK, index >> S32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    k = np.searchsorted(thresholds(lam), words[0], side='right').astype(np.int64)        # the number of T_j <= u
    minus = (words[sign_word] >> np.uint64(31)).astype(bool)
    return np.where(minus, -k, k).reshape(h, w)


def poisson_noise(img: np.ndarray, lam: int, seed: int) -> np.ndarray:
    """The operator on uint8 [h, w, 3]."""
    n = noise_field(img.shape[0], img.shape[1], lam, seed)
    return np.clip(img.astype(np.int64) + n[..., None], 0, 255).astype(np.uint8)


# ---- mutants: each breaks one clause of the definition --------------------------------------------------------------------------
def mutant_lam_plus_one(img, lam, seed):
    return poisson_noise(img, lam + 1, seed)


def mutant_no_sign(img, lam, seed):
    n = np.abs(noise_field(img.shape[0], img.shape[1], lam, seed))
    return np.clip(img.astype(np.int64) + n[..., None], 0, 255).astype(np.uint8)


def mutant_independent_channels(img, lam, seed):
    n = np.stack([noise_field(img.shape[0], img.shape[1], lam, seed + c) for c in range(3)], axis=-1)
    return np.clip(img.astype(np.int64) + n, 0, 255).astype(np.uint8)


def mutant_one_word(img, lam, seed):
    """Word 1 gives both the uniform and the sign: the sign is the uniform's top bit, so small k are all positive."""
    h, w = img.shape[:2]
    index = np.arange(h * w, dtype=np.uint64)
    words = philox4x32_10((index & MASK, index >> S32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    k = np.searchsorted(thresholds(lam), words[1], side='right').astype(np.int64)
    n = np.where((words[1] >> np.uint64(31)).astype(bool), -k, k).reshape(h, w)
    return np.clip(img.astype(np.int64) + n[..., None], 0, 255).astype(np.uint8)


MUTANTS = {'lam + 1': mutant_lam_plus_one, 'no sign': mutant_no_sign, 'independent channels': mutant_independent_channels,
           'word 1 for both draws': mutant_one_word}
