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
10 x 512 form: one (round, chunk) block of a larger size through the NumPy-mode kernel.

Any RECIPE (`Recipe`: a list of 1..12 kinds, the positions of a round, and six strengths; the above is the default one): view v
is of the kind at position v % L in round v // L, and the counter slots follow from the list by one rule (`Recipe.table`), so A
VIEW'S DRAWS DEPEND ON THE KINDS BEFORE IT IN THE LIST -- the price of leaving the default layout untouched.  `views` is the
pure-NumPy statement of a clip's expected views by a recipe; the kernels are held to it."""
import math

import numpy as np

from ._lib import VIEW_KINDS, VIEW_POS_MAX, VIEW_TABLE_COLS
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


def counters(num_crop=NUM_CROP, num_point=NUM_POINT, recipe=None):
    """Every counter word the recipe reads, by user: {(view, purpose): set of (n, slot, word)} with purpose 'row',
    ('jitter', j, d) or 'angle' (the scalar draw of a rot or scale view).  (clip id and epoch are the same in every counter
    of a clip's views.)  `recipe` None: the default recipe, whose layout is the literal one above."""
    check_size(num_crop, num_point)
    out = {}
    if recipe is not None:
        table, stride = recipe.table()
        for v in range(num_crop):
            t, s0 = table[v % len(table)], stride * (v // len(table))
            out[(v, 'row')] = {(n, s0 + int(t[T_ROW_SLOT]), int(t[T_ROW_WORD])) for n in range(num_point)}
            for j in (int(t[T_JIT0]), int(t[T_JIT1])):
                for d in range(3 if j >= 0 else 0):
                    out[(v, ('jitter', j, d))] = {(n, s0 + 3 + 3 * j + d, w) for n in range(num_point) for w in (0, 1)}
            if t[T_SCALAR] >= 0:
                out[(v, 'angle')] = {(0, s0 + int(t[T_SCALAR]), w) for w in (0, 1)}
        return out
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


# ---- the recipe: which kinds a round holds and how strongly they are augmented (include/facl_hip.h) ----------
KIND_NAMES = VIEW_KINDS                                   # name -> code: its index (FACL_VIEW_<NAME>)
REFERENCE_KINDS = ("raw", "mirror", "key", "key_mirror", "rot", "rot", "t4", "t7", "res30", "res10")
STRENGTH_NAMES = ("jitter_sigma", "jitter_clip", "rot_range", "scale_lo", "scale_hi", "tilt_angle")
DEFAULT_STRENGTHS = (0.01, 0.05, 0.8, 0.5, 1.5, 0.25)     # the reference's literals (:767, :739, :759, :723)
# columns of a position's descriptor (facl_view_recipe_table)
T_SRC, T_CH, T_OP, T_ROW_SLOT, T_ROW_WORD, T_JIT0, T_JIT1, T_SCALAR = range(VIEW_TABLE_COLS)
OP_GATHER, OP_JITTER, OP_MIRROR, OP_ROT, OP_SCALE, OP_TILT_NEG, OP_TILT_POS = range(7)
#          kind:  raw        mirror      key         key_mirror  rot        t4         t7         res30      res10
_DESCRIPTOR = ((0, 3, 0), (0, 3, 2), (1, 3, 1), (1, 3, 2), (0, 3, 3), (4, 4, 0), (5, 7, 0), (2, 3, 0), (3, 3, 0),
               (0, 3, 1), (0, 3, 4), (0, 3, 5), (0, 3, 6))   # jitter, scale, tilt_neg, tilt_pos: (source, channel, operation)


class Recipe:
    """A list of 1..12 kinds (the positions of a round) and six strengths.  View v is of the kind at position v % L in round
    v // L.  The counter slots follow from the list by one rule (`table`), so a view's draws depend on the kinds before it in
    the list; the default list gives the layout the ten reference views always had."""

    def __init__(self, kinds=REFERENCE_KINDS, **strengths):
        kinds = tuple(kinds)
        if not 1 <= len(kinds) <= VIEW_POS_MAX:
            raise ValueError("--view_kinds: a recipe lists 1..%d kinds (got %d)" % (VIEW_POS_MAX, len(kinds)))
        for k in kinds:
            if k not in KIND_NAMES:
                raise ValueError("--view_kinds: unknown kind %r (the kinds: %s; 'reference' = %s)"
                                 % (k, ", ".join(KIND_NAMES), ",".join(REFERENCE_KINDS)))
        unknown = set(strengths) - set(STRENGTH_NAMES)
        if unknown:
            raise TypeError("unknown strength %s" % ", ".join(sorted(unknown)))
        self.kinds = kinds
        for name, default in zip(STRENGTH_NAMES, DEFAULT_STRENGTHS):
            v = float(strengths.get(name, default))
            if not np.isfinite(v):
                raise ValueError("--%s must be finite (got %r)" % (name, v))
            setattr(self, name, v)
        if self.jitter_sigma < 0:
            raise ValueError("--jitter_sigma must be >= 0 (got %r)" % self.jitter_sigma)
        if self.jitter_clip <= 0:
            raise ValueError("--jitter_clip must be > 0 (got %r; the reference asserts clip > 0)" % self.jitter_clip)
        if not 0 <= self.rot_range <= 2:
            raise ValueError("--rot_range must be in [0, 2] (got %r): the angle is (u - 0.5) * pi * rot_range" % self.rot_range)
        if self.scale_lo <= 0:
            raise ValueError("--scale_lo must be > 0 (got %r)" % self.scale_lo)
        if self.scale_lo > self.scale_hi:
            raise ValueError("--scale_hi must be >= --scale_lo (got %r < %r)" % (self.scale_hi, self.scale_lo))

    @classmethod
    def parse(cls, text, **strengths):
        """'raw,mirror,scale' -> Recipe; the name 'reference' stands for the default list."""
        names = []
        for part in str(text).split(","):
            part = part.strip()
            if part:
                names.extend(REFERENCE_KINDS if part == "reference" else (part,))
        return cls(names, **strengths)

    def codes(self):
        return np.array([KIND_NAMES.index(k) for k in self.kinds], dtype=np.int32)

    def strengths(self):
        return np.array([getattr(self, n) for n in STRENGTH_NAMES], dtype=np.float64)

    def is_default(self):
        return self.kinds == REFERENCE_KINDS and tuple(self.strengths()) == DEFAULT_STRENGTHS

    def table(self):
        """((L, 8) int32 descriptors, stride): per position source, channel, operation, row slot, row word, first / second
        jitter draw j (-1: none), scalar slot (-1: none); stride = the counter slots of a round."""
        ops = [_DESCRIPTOR[c][2] for c in self.codes()]
        J = sum(2 if op == OP_MIRROR else (1 if op != OP_GATHER else 0) for op in ops)
        scalar0 = 3 + 3 * max(7, J)
        t = np.full((len(ops), VIEW_TABLE_COLS), -1, dtype=np.int32)
        j = a = 0
        for i, c in enumerate(self.codes()):
            t[i, :5] = _DESCRIPTOR[c] + (i >> 2, i & 3)
            if ops[i] != OP_GATHER:
                t[i, T_JIT0], j = j, j + 1
            if ops[i] == OP_MIRROR:
                t[i, T_JIT1], j = j, j + 1
            if ops[i] in (OP_ROT, OP_SCALE):
                t[i, T_SCALAR], a = scalar0 + a, a + 1
        return t, 32 * -(-(scalar0 + a) // 32)

    def describe(self):
        return "view recipe: %s | %s" % (",".join(self.kinds),
                                         " ".join("%s %g" % (n, getattr(self, n)) for n in STRENGTH_NAMES))

    def __eq__(self, other):
        return isinstance(other, Recipe) and self.kinds == other.kinds and tuple(self.strengths()) == tuple(other.strengths())

    def __hash__(self):
        return hash((self.kinds, tuple(self.strengths())))


# the arithmetic of the operations, each in the reference's dtype walk (S = the source dtype, float32 or float64)
def jitter_op(x, z, sigma=0.01, clip=0.05):
    """jitter_point_cloud (:767-778) written back into the source array: S(double(x) + clip(sigma z, +-clip))."""
    return (x.astype(np.float64) + np.clip(sigma * np.asarray(z, dtype=np.float64), -clip, clip)).astype(x.dtype)


def mirror_op(x, z, sigma=0.01, clip=0.05):
    """reverse_transform (:708-713): a float32 copy, x negated, a second jitter rounded to float32."""
    f = x.astype(np.float32)
    f[:, 0] = -f[:, 0]
    return jitter_op(f, z, sigma, clip)


def rotate_y_op(x, c, s):
    """rotate_trans / depth_transform (:716-749): a float32 copy times Ry in fp64, rounded to float32."""
    f = x.astype(np.float32).astype(np.float64)
    return np.stack((f[:, 0] * c + f[:, 2] * (-s), f[:, 1], f[:, 0] * s + f[:, 2] * c), -1).astype(np.float32)


def scale_op(x, factor):
    """scale_trans (:757-763): a Python-float factor times an S array is an S product; float32 at the end."""
    return (x.dtype.type(factor) * x).astype(np.float32)


def tilt_cos_sin(tilt_angle):
    """cos / sin of +pi * tilt_angle as the host passes them to the kernel (the C library's, as math's are)."""
    return math.cos(math.pi * tilt_angle), math.sin(math.pi * tilt_angle)


def views(recipe, seed, epoch, clip_id, clip, num_crop=NUM_CROP, num_point=NUM_POINT):
    """The expected views of one clip by `recipe`, pure NumPy: ((G, P, 4) float32, (G, P) int64 rows of the view's source
    cloud -- of the point cloud for the temporal kinds; -1 and zeros where a temporal view cannot be drawn).  `clip`: the
    four (rows, >= 8) source clouds.  The kernels are held to this."""
    check_size(num_crop, num_point)
    recipe = Recipe() if recipe is None else recipe
    table, stride = recipe.table()
    G, P, L = int(num_crop), int(num_point), len(table)
    n = np.arange(P, dtype=np.uint64)
    out = np.zeros((G, P, 4), dtype=np.float32)
    rows = np.full((G, P), -1, dtype=np.int64)
    sigma, clip_at = recipe.jitter_sigma, recipe.jitter_clip

    for v in range(G):
        t, s0 = table[v % L], stride * (v // L)
        word = _words(seed, s0 + int(t[T_ROW_SLOT]), clip_id, epoch, n)[:, int(t[T_ROW_WORD])]
        if t[T_SRC] >= 4:
            cloud = clip[0]
            nz = np.flatnonzero(cloud[:, int(t[T_CH])] != 0)
            if nz.shape[0] == 0:
                continue                                      # a void view
            row = nz[row_draw(word, nz.shape[0])]
        else:
            cloud = clip[int(t[T_SRC])]
            row = row_draw(word, cloud.shape[0])
        rows[v] = row
        x = cloud[row, :3].copy()
        out[v, :, 3] = cloud[row, int(t[T_CH])]

        def z(j):
            w = [_words(seed, s0 + 3 + 3 * j + d, clip_id, epoch, n) for d in range(3)]
            return np.stack([normal(wd[:, 0], wd[:, 1]) for wd in w], -1)

        def u():
            w = _words(seed, s0 + int(t[T_SCALAR]), clip_id, epoch, n=[0])[0]
            return float(uniform53(w[0:1], w[1:2])[0])

        op = int(t[T_OP])
        if op != OP_GATHER:
            x = jitter_op(x, z(int(t[T_JIT0])), sigma, clip_at)
        if op == OP_MIRROR:
            x = mirror_op(x, z(int(t[T_JIT1])), sigma, clip_at)
        elif op == OP_ROT:
            angle = (u() - 0.5) * np.pi * recipe.rot_range
            x = rotate_y_op(x, np.cos(angle), np.sin(angle))
        elif op in (OP_TILT_NEG, OP_TILT_POS):
            c, s = tilt_cos_sin(recipe.tilt_angle)
            x = rotate_y_op(x, c, -s if op == OP_TILT_NEG else s)
        elif op == OP_SCALE:
            x = scale_op(x, recipe.scale_lo + (recipe.scale_hi - recipe.scale_lo) * u())
        out[v, :, :3] = x.astype(np.float32)
    return out, rows
