"""NumPy restatement of the counter-based draws of --view_rng philox (csrc/views_philox.hip; the recipe is in that file's
header).  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011), vectorised over counters.
`draws` returns exactly what facl_amd.views.draw_clip returns for one clip, so that the philox draws fed through the
NumPy-mode kernel (csrc/views.hip) give the philox kernel's views: the tests compare the two."""
import numpy as np

from .views import NUM_CROP, NUM_POINT

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter (..., 4) uint32-valued, key (2,) ints -> (..., 4) uint32 words."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & _MASK for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _words(seed, slot, clip_id, epoch, n=None):
    n = np.arange(NUM_POINT, dtype=np.uint64) if n is None else np.asarray(n, dtype=np.uint64)
    ctr = np.stack([n, np.full_like(n, slot), np.full_like(n, clip_id & 0xFFFFFFFF), np.full_like(n, epoch & 0xFFFFFFFF)], -1)
    return philox4x32_10(ctr, seed_key(seed))


def row_draw(w, count):
    """(uint64(w) * count) >> 32: uniform in [0, count)."""
    return ((w.astype(np.uint64) * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def normal(w0, w1):
    """Box-Muller from two words, fp64: u1 in (0, 1], u2 in [0, 1)."""
    u1 = (w0.astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = w1.astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def uniform53(w0, w1):
    return ((w0 >> np.uint32(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53


def draws(seed, epoch, clip_id, points, key_points, res_points_1, res_points_2, base):
    """The philox draws of one clip in draw_clip's form: (idx (10,512) int32 absolute rows, noise (7,512,3) float64,
    cossin (2,2) float64).  `base` = row offsets of the four source clouds in the packed batch buffer."""
    sizes = (points.shape[0], key_points.shape[0], res_points_1.shape[0], res_points_2.shape[0])
    src_of = (0, 0, 1, 1, 0, 0, None, None, 2, 3)
    rw = np.concatenate([_words(seed, s, clip_id, epoch) for s in range(3)], -1)      # (512, 12): view v = word v
    idx = np.empty((NUM_CROP, NUM_POINT), dtype=np.int64)
    for v in range(NUM_CROP):
        if src_of[v] is None:
            nz = np.flatnonzero(points[:, 4 if v == 6 else 7] != 0)
            if nz.shape[0] == 0:
                raise ValueError("no row with a non-zero channel %d" % (4 if v == 6 else 7))
            idx[v] = base[0] + nz[row_draw(rw[:, v], nz.shape[0])]
        else:
            idx[v] = base[src_of[v]] + row_draw(rw[:, v], sizes[src_of[v]])
    noise = np.empty((7, NUM_POINT, 3), dtype=np.float64)
    for j in range(7):
        for d in range(3):
            w = _words(seed, 3 + 3 * j + d, clip_id, epoch)
            noise[j, :, d] = normal(w[:, 0], w[:, 1])
    cs = np.empty((2, 2), dtype=np.float64)
    for k in range(2):
        w = _words(seed, 24 + k, clip_id, epoch, n=[0])[0]
        angle = (uniform53(w[0:1], w[1:2])[0] - 0.5) * np.pi * 0.8
        cs[k] = (np.cos(angle), np.sin(angle))
    return idx.astype(np.int32), noise, cs
