"""NumPy restatement of the counter-based draws of --view_rng philox (csrc/views_philox.hip; the recipe is in that file's
header).  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011), vectorised over counters.
`draws` returns exactly what facl_amd.views.draw_clip returns for one clip, so that the philox draws fed through the
NumPy-mode kernel (csrc/views.hip) give the philox kernel's views: the tests compare the two.

Any view count G and cloud size P (an extension: the reference's loader has 10 x 512 only).  View v is of KIND k = v % 10
(raw, reversed, key, key-reversed, rotated x2, temporal channel 4, temporal channel 7, low-res x2) in ROUND r = v // 10.
Every counter keeps the form (point n, slot, clip id, epoch); the slot of round r is the kind's slot + 32 * r (a round uses
slots 0..25: rows 0..2, jitter 3..23, angles 24, 25), so the row word of view v is word k & 3 of slot (k >> 2) + 32 * r.  The
point index n runs over 0..P-1.  Domain: 1 <= G <= 64; 64 <= P <= 4096, P % 64 == 0 (the grouping limit).  Hence a view's
values do not depend on G, its first P' points do not depend on P, and the block [v < 10, n < 512] of any size is the 10 x 512
output bit for bit.  `draws(..., round=r, first_point=f)` returns the draws of round r for points f .. f+511 in draw_clip's
10 x 512 form: one (round, chunk) block of a larger size through the NumPy-mode kernel."""
import numpy as np

from .views import NUM_CROP, NUM_POINT, check_view_size as check_size

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


KINDS = NUM_CROP               # views of a round
ROUND_SLOTS = 32               # counter slots per round
_JITTER_OF = {1: (0, 1), 2: (2,), 3: (3, 4), 4: (5,), 5: (6,)}      # kind -> its jitter slots (csrc/views.hip's j)


def counters(num_crop=NUM_CROP, num_point=NUM_POINT):
    """Every counter word the recipe reads, by user: {(view, purpose): set of (n, slot, word)} with purpose 'row',
    ('jitter', j, d) or 'angle'.  (clip id and epoch are the same in every counter of a clip's views.)"""
    check_size(num_crop, num_point)
    out = {}
    for v in range(num_crop):
        k, s0 = v % KINDS, ROUND_SLOTS * (v // KINDS)
        out[(v, 'row')] = {(n, s0 + (k >> 2), k & 3) for n in range(num_point)}
        for j in _JITTER_OF.get(k, ()):
            for d in range(3):
                out[(v, ('jitter', j, d))] = {(n, s0 + 3 + 3 * j + d, w) for n in range(num_point) for w in (0, 1)}
        if k in (4, 5):
            out[(v, 'angle')] = {(0, s0 + 24 + (k - 4), w) for w in (0, 1)}
    return out


def draws(seed, epoch, clip_id, points, key_points, res_points_1, res_points_2, base, num_crop=NUM_CROP,
          num_point=NUM_POINT, round=0, first_point=0):
    """The philox draws of one clip in draw_clip's form: (idx (10,512) int32 absolute rows, noise (7,512,3) float64,
    cossin (2,2) float64).  `base` = row offsets of the four source clouds in the packed batch buffer.  With `num_crop`
    views of `num_point` points: the draws of views 10*round .. 10*round+9 for points first_point .. first_point+511 (the
    values depend on neither size; kinds past num_crop and points past num_point are drawn all the same and unused)."""
    check_size(num_crop, num_point)
    if not (0 <= round <= (num_crop - 1) // KINDS) or not (0 <= first_point < num_point):
        raise ValueError("round %r / first_point %r outside %d views of %d points" % (round, first_point, num_crop, num_point))
    s0 = ROUND_SLOTS * round
    pts = first_point + np.arange(NUM_POINT, dtype=np.uint64)
    sizes = (points.shape[0], key_points.shape[0], res_points_1.shape[0], res_points_2.shape[0])
    src_of = (0, 0, 1, 1, 0, 0, None, None, 2, 3)
    rw = np.concatenate([_words(seed, s0 + s, clip_id, epoch, pts) for s in range(3)], -1)   # (512, 12): kind k = word k
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
            w = _words(seed, s0 + 3 + 3 * j + d, clip_id, epoch, pts)
            noise[j, :, d] = normal(w[:, 0], w[:, 1])
    cs = np.empty((2, 2), dtype=np.float64)
    for k in range(2):
        w = _words(seed, s0 + 24 + k, clip_id, epoch, n=[0])[0]
        angle = (uniform53(w[0:1], w[1:2])[0] - 0.5) * np.pi * 0.8
        cs[k] = (np.cos(angle), np.sin(angle))
    return idx.astype(np.int32), noise, cs
