// What the three view kernels share: csrc/views.hip (NumPy's draws, made on the host), csrc/views_philox.hip (counter-based
// draws, a packed batch from disk) and csrc/views_resident.hip (counter-based draws, clips selected by index out of a pool
// resident in device memory).  Here live the Philox4x32-10 block, the draw recipe (which word of which counter picks the row
// of a view's point, the Box-Muller jitter, the rotation angle), the dtype walk of the arithmetic, the body of the two
// gather kernels (build_view) and the tail of their launchers (view_launch).  The kernels differ only in where a random
// number comes from and in how a drawn position becomes a row of their source array; everything a view's VALUES depend on
// lives here, so the paths cannot drift apart (their views are required to be equal bit for bit).  The arithmetic is stated
// TWICE, not once: view_chain_reference, the reference's ten views as an if-chain (what views.hip runs, and the philox
// kernels at the default recipe: REF = true), and view_point, the table-driven form of any recipe.  Both stay because the
// table-driven form measured slower at the default recipe (DESIGN 3.10.1); tests/test_gpu_view_recipe.py holds the two to
// each other bit for bit.  Include inside an anonymous namespace, after common.h.  The recipe is restated in NumPy by
// facl_amd/philox.py, which the tests hold the kernels to, and in include/facl_hip.h for the callers of the C ABI.
//
// Draw recipe of the counter-based views, written for the first ten views ("views 0..9" below are the ten KINDS: raw,
// reversed, key, key-reversed, rotated x2, temporal channel 4, temporal channel 7, low-res x2):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (point n in 0..P-1, slot, clip id, epoch)           -> four 32-bit words w0..w3
//   rows    slot 0: views 0,1,2,3 = w0..w3; slot 1: views 4,5,6,7; slot 2: views 8,9 = w0,w1.
//           row = (uint64(w) * count) >> 32 in [0, count) of the view's source cloud (views 6, 7: of the list of rows
//           whose channel 4 / 7 is non-zero, compacted by the temporal-rows kernels)
//   jitter  slot 3 + 3*j + d (j = jitter slot 0..6: rev 0,1 | ke1 2 | ke2 3,4 | ro1 5 | ro2 6; d = xyz): u1 = (w0 + 1) * 2^-32
//           in (0, 1], u2 = w1 * 2^-32 in [0, 1), z = sqrt(-2 log u1) * cos(2 pi u2) in fp64, then clip(0.01 z, -0.05, 0.05)
//   angle k (k = 0, 1; views 4, 5): counter (0, 24 + k, clip id, epoch), u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53,
//           angle = (u - 0.5) * pi * 0.8, cos / sin in fp64
// Any G and P (the reference has no recipe beyond 10 x 512: an extension, on this stream only):
//   view v  is of kind k = v % 10 in round r = v / 10 and draws as kind k does, with EVERY slot moved by 32 * r: its row
//           word is word k & 3 of slot (k >> 2) + 32 r, its jitter slots are 3 + 3 j + d + 32 r, its angle slot 24 + (k - 4)
//           + 32 r.  Slots 0..25 of a round are in use, so rounds never share a counter.
//   point n runs over 0..P-1 in counter word 0; nothing else changes.
//   domain  1 <= G <= 64; 64 <= P <= 4096 with P % 64 == 0 (the grouping limit); FACL_E_SHAPE otherwise.
// So a view's values do not depend on G, its first P' points do not depend on P, and G = 10, P = 512 -- the entries
// without _gp, which call the same launcher -- is the block [v < 10, n < 512] of every other size, bit for bit.
// Any RECIPE (a list of L = 1..12 kinds, the positions of a round, and six strengths; the text above is the default one):
//   view v  is of the kind at position v % L in round v / L; every slot of round r is the position's slot + stride * r.
//   kinds   raw, mirror, key, key_mirror, rot, t4, t7, res30, res10 (above); jitter = points, jitter; scale = points, jitter,
//           xyz * s; tilt_neg / tilt_pos = points, jitter, rotation about y by -/+ pi * tilt_angle (cn3D_data_set.py:356-358,
//           :697-704 then :757-763 / :716-732)
//   slots   row word of position i: word i & 3 of slot i >> 2.  Jitter draws are numbered j = 0, 1, ... in position order
//           (mirror, key_mirror: two; key, rot, jitter, scale, tilt_*: one) and draw j uses slots 3 + 3 j + d.  Scalar draws (rot,
//           scale: one each) are numbered in position order from 3 + 3 max(7, J), J = jitter draws of the round.  stride =
//           32 ceil((3 + 3 max(7, J) + A) / 32), A = scalar draws.  The default list gives the layout above (j = 0..6, scalars
//           24, 25, stride 32).  So a view's draws depend on the kinds BEFORE it in the list.
//   dtype walk (S = source dtype):
//     jitter  before any float32 operation: x = S(double(x) + clip(jitter_sigma * z, +-jitter_clip)), jit()'s evaluation
//             order (0.01 / 0.05 give the earlier bits); the second jitter of the mirrored kinds on float32
//     rot     on double(float(x)): fx c + fz (-s), fy, fx s + fz c, rounded to float32; angle = ((u - 0.5) * pi) * rot_range
//     tilt_*  the same rotation with cos / sin of pi * tilt_angle, computed once on the host and passed by value
//     scale   s = scale_lo + (scale_hi - scale_lo) * u in fp64 as written (contraction off), rounded to S; the product in S,
//             cast to float32 (NumPy with a Python-float factor and an S array); u = uniform53 of the position's scalar slot
// The host derives a descriptor per position (view_recipe_make) and the kernels take the whole recipe BY VALUE in their
// arguments: no device allocation, no copy, no launch of its own.  REF = true is the default recipe folded into the code.

constexpr int KINDS = 10;                 // the reference's ten views = the positions of a round of the default recipe
constexpr int ROUND_SLOTS = 32;           // counter slots per round of the default recipe (a recipe's own: its stride)
constexpr int CHUNK = 512;                // points per workgroup at most (the reference's cloud: one workgroup per view)
constexpr int G_MAX = 64, P_MIN = 64, P_MAX = 4096;
constexpr int TR_THREADS = 256;           // temporal-row compaction: 4 waves, 256 rows per pass

// what a position does with its gathered row (after the first jitter, which every operation but OP_GATHER starts with)
enum { OP_GATHER = 0, OP_JITTER, OP_MIRROR, OP_ROT, OP_SCALE, OP_TILT_NEG, OP_TILT_POS };
// where its row comes from: the four source clouds, or the rows of the point cloud with a non-zero channel 4 / 7
enum { SRC_POINTS = 0, SRC_KEY, SRC_RES1, SRC_RES2, SRC_T4, SRC_T7 };

// one position of a round; slots are relative to the round's first.  jit0 / jit1: the jitter draw j (slots 3 + 3 j + d)
struct ViewPos { uint8_t src, ch, op, row_slot, row_word, jit0, jit1, scalar; };

struct ViewRecipe {
    int n, stride;                        // positions of a round; counter slots per round
    ViewPos pos[FACL_VIEW_POS_MAX];
    double sigma, clip, rot_range, scale_lo, scale_hi, tilt_cos, tilt_sin;     // cos / sin of +pi * tilt_angle
};

constexpr int32_t DEFAULT_KINDS[KINDS] = {FACL_VIEW_RAW, FACL_VIEW_MIRROR, FACL_VIEW_KEY, FACL_VIEW_KEY_MIRROR, FACL_VIEW_ROT,
                                          FACL_VIEW_ROT, FACL_VIEW_T4, FACL_VIEW_T7, FACL_VIEW_RES30, FACL_VIEW_RES10};
constexpr double DEFAULT_STRENGTHS[FACL_VIEW_NSTRENGTH] = {0.01, 0.05, 0.8, 0.5, 1.5, 0.25};

// The slot rule ("slots" in the header), host side.  table (n_kinds, FACL_VIEW_TABLE_COLS) int32 per position: source,
// channel, operation, row slot, row word, first / second jitter draw j (-1: none), scalar slot (-1: none).  For the default
// list this is the layout the kernels always had: j = 0..6 on positions 1, 1, 2, 3, 3, 4, 5, scalars 24, 25, stride 32.
static inline int view_recipe_table(const int32_t* kinds, int n_kinds, int32_t* table, int32_t* stride) {
    if (!kinds || !table || !stride) return FACL_E_NULL;
    if (n_kinds < 1 || n_kinds > FACL_VIEW_POS_MAX) return FACL_E_SHAPE;
    int J = 0, A = 0;
    for (int i = 0; i < n_kinds; ++i) {
        const int k = kinds[i];
        if (k < 0 || k >= FACL_VIEW_NKINDS) return FACL_E_SHAPE;
        J += (k == FACL_VIEW_MIRROR || k == FACL_VIEW_KEY_MIRROR) ? 2
             : (k == FACL_VIEW_KEY || k == FACL_VIEW_ROT || k >= FACL_VIEW_JITTER) ? 1 : 0;
    }
    const int scalar0 = 3 + 3 * (J > 7 ? J : 7);
    int j = 0;
    for (int i = 0; i < n_kinds; ++i) {
        const int k = kinds[i];
        int32_t* t = table + i * FACL_VIEW_TABLE_COLS;
        int src = SRC_POINTS, ch = 3, op = OP_GATHER;
        switch (k) {
            case FACL_VIEW_MIRROR: op = OP_MIRROR; break;
            case FACL_VIEW_KEY: src = SRC_KEY; op = OP_JITTER; break;
            case FACL_VIEW_KEY_MIRROR: src = SRC_KEY; op = OP_MIRROR; break;
            case FACL_VIEW_ROT: op = OP_ROT; break;
            case FACL_VIEW_T4: src = SRC_T4; ch = 4; break;
            case FACL_VIEW_T7: src = SRC_T7; ch = 7; break;
            case FACL_VIEW_RES30: src = SRC_RES1; break;
            case FACL_VIEW_RES10: src = SRC_RES2; break;
            case FACL_VIEW_JITTER: op = OP_JITTER; break;
            case FACL_VIEW_SCALE: op = OP_SCALE; break;
            case FACL_VIEW_TILT_NEG: op = OP_TILT_NEG; break;
            case FACL_VIEW_TILT_POS: op = OP_TILT_POS; break;
            default: break;                                       // FACL_VIEW_RAW
        }
        t[0] = src; t[1] = ch; t[2] = op; t[3] = i >> 2; t[4] = i & 3;
        t[5] = op != OP_GATHER ? j++ : -1;
        t[6] = op == OP_MIRROR ? j++ : -1;
        t[7] = (op == OP_ROT || op == OP_SCALE) ? scalar0 + A++ : -1;
    }
    *stride = 32 * ((scalar0 + A + 31) / 32);
    return 0;
}

// the recipe a kernel takes, from the caller's HOST arrays; every refusal of the C ABI's recipe entries is made here
static inline int view_recipe_make(const int32_t* kinds, int n_kinds, const double* st, ViewRecipe* rc) {
    if (!kinds || !st) return FACL_E_NULL;
    int32_t table[FACL_VIEW_POS_MAX * FACL_VIEW_TABLE_COLS], stride = 0;
    const int e = view_recipe_table(kinds, n_kinds, table, &stride);
    if (e != 0) return e;
    for (int i = 0; i < FACL_VIEW_NSTRENGTH; ++i)
        if (!std::isfinite(st[i])) return FACL_E_SHAPE;
    if (st[0] < 0.0 || st[1] <= 0.0 || st[2] < 0.0 || st[2] > 2.0 || st[3] <= 0.0 || st[3] > st[4]) return FACL_E_SHAPE;
    *rc = ViewRecipe{};
    rc->n = n_kinds;
    rc->stride = stride;
    for (int i = 0; i < n_kinds; ++i) {
        const int32_t* t = table + i * FACL_VIEW_TABLE_COLS;
        rc->pos[i] = {(uint8_t)t[0], (uint8_t)t[1], (uint8_t)t[2], (uint8_t)t[3], (uint8_t)t[4], (uint8_t)t[5], (uint8_t)t[6],
                      (uint8_t)t[7]};
    }
    rc->sigma = st[0]; rc->clip = st[1]; rc->rot_range = st[2]; rc->scale_lo = st[3]; rc->scale_hi = st[4];
    const double tilt = 3.141592653589793 * st[5];
    rc->tilt_cos = std::cos(tilt);
    rc->tilt_sin = std::sin(tilt);
    return 0;
}

static inline ViewRecipe view_recipe_default() {
    ViewRecipe rc;
    view_recipe_make(DEFAULT_KINDS, KINDS, DEFAULT_STRENGTHS, &rc);
    return rc;
}

struct u32x4 { uint32_t w[4]; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ int draw_row(uint32_t w, int count) {
    return (int)(((unsigned long long)w * (unsigned long long)(uint32_t)count) >> 32);
}

__device__ __forceinline__ double jit(double n, double sigma, double clip) {      // np.clip(sigma * n, -clip, clip)
    const double v = sigma * n;
    return v < -clip ? -clip : (v > clip ? clip : v);
}

// what a (clip, view, point) draws with: the key, the clip's dataset index and the epoch
struct ViewDraw { uint32_t k0, k1, cid, epoch; };

__device__ __forceinline__ ViewDraw view_draw(int64_t seed, uint32_t cid, int epoch) {
    const uint64_t s = (uint64_t)seed;
    return {(uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32), cid, (uint32_t)epoch};
}

// the domain of (G, P): 1..64 views; 64..4096 points in whole waves (the upper bound is the grouping limit)
static inline bool views_gp_ok(int G, int P) {
    return G >= 1 && G <= G_MAX && P >= P_MIN && P <= P_MAX && P % FACL_WAVE == 0;
}

// launch geometry: workgroups of (clip, view, chunk of up to 512 points), `threads` points each
struct ViewGrid { int threads, chunks; };
static inline ViewGrid view_grid(int P) {
    const int threads = P < CHUNK ? P : CHUNK;
    return {threads, (P + threads - 1) / threads};
}

// where a workgroup stands: clip b of the batch, view v = position k of the round whose first slot is slot0, point n
// (n >= P: nothing to do).  b, v, k and slot0 are uniform across the workgroup.
struct ViewAt { int b, v, k, slot0, n; };

__device__ __forceinline__ ViewAt view_at(const ViewRecipe& rc, int G, int chunks) {
    const int c = (int)blockIdx.x % chunks, bv = (int)blockIdx.x / chunks;
    const int v = bv % G, round = v / rc.n;
    return {bv / G, v, v - round * rc.n, rc.stride * round, c * (int)blockDim.x + (int)threadIdx.x};
}

// the 32-bit word that picks the source row of point n of a view at position d: draw_row(word, count) in [0, count)
__device__ __forceinline__ uint32_t view_row_word(const ViewDraw& q, const ViewPos& d, int slot0, int n) {
    const u32x4 rw = philox4x32_10((uint32_t)n, (uint32_t)(slot0 + d.row_slot), q.cid, q.epoch, q.k0, q.k1);
    return rw.w[d.row_word];
}

// standard normal of jitter draw j, coordinate d, of point n: Box-Muller on words 0, 1 of slot 3 + 3 j + d
__device__ __forceinline__ double draw_normal(const ViewDraw& q, int slot0, int n, int j, int d) {
    const u32x4 p = philox4x32_10((uint32_t)n, (uint32_t)(slot0 + 3 + 3 * j + d), q.cid, q.epoch, q.k0, q.k1);
    const double u1 = ((double)p.w[0] + 1.0) * 0x1p-32, u2 = (double)p.w[1] * 0x1p-32;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// a scalar draw, one per (clip, view): 53 uniform bits of words 0, 1 of `slot`, in [0, 1)
__device__ __forceinline__ double draw_uniform53(const ViewDraw& q, int slot) {
    const u32x4 p = philox4x32_10(0u, (uint32_t)slot, q.cid, q.epoch, q.k0, q.k1);
    return ((double)(p.w[0] >> 5) * 67108864.0 + (double)(p.w[1] >> 6)) * 0x1p-53;
}

__device__ __forceinline__ void view_void(float* dst) {    // a view that cannot be drawn: zeros
    *reinterpret_cast<float4*>(dst) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// point n of a view at position d (slots from slot0 = stride * round) from its source row r (>= 8 channels): jitter in
// fp64 written back in the source dtype, mirror / rotation on float32, scale in the source dtype, channel select; one
// float4 store to dst
template <typename S>
__device__ __forceinline__ void view_point(const S* __restrict__ r, const ViewDraw& q, const ViewRecipe& rc, const ViewPos& d,
                                           int slot0, int n, float* __restrict__ dst) {
    const double sigma = rc.sigma, clip = rc.clip;
    const int op = d.op;
    S x[3] = {r[0], r[1], r[2]};
    const S w = r[d.ch];
    float o[4];
    o[3] = (float)w;
    auto jz = [&](int j, int dd) { return jit(draw_normal(q, slot0, n, j, dd), sigma, clip); };
    auto uniform53 = [&] { return draw_uniform53(q, slot0 + d.scalar); };      // the position's scalar draw
    auto rotate = [&](double c, double s) {                    // about y, on float32 coordinates (:716-732, :734-749)
        const double fx = (double)(float)x[0], fy = (double)(float)x[1], fz = (double)(float)x[2];
        o[0] = (float)(fx * c + fz * (-s));
        o[1] = (float)fy;
        o[2] = (float)(fx * s + fz * c);
    };
    if (op != OP_GATHER) {                                     // every other operation starts with the jitter (:767-778)
#pragma unroll
        for (int dd = 0; dd < 3; ++dd) x[dd] = (S)((double)x[dd] + jz(d.jit0, dd));
    }
    if (op == OP_MIRROR) {                                     // reverse_transform (:708-713)
        float f[3] = {(float)x[0], (float)x[1], (float)x[2]};
        f[0] = -f[0];
#pragma unroll
        for (int dd = 0; dd < 3; ++dd) o[dd] = (float)((double)f[dd] + jz(d.jit1, dd));
    } else if (op == OP_ROT) {                                 // rotate_trans (:734-749)
        const double angle = (uniform53() - 0.5) * 3.141592653589793 * rc.rot_range;
        rotate(cos(angle), sin(angle));
    } else if (op == OP_TILT_NEG || op == OP_TILT_POS) {       // depth_transform (:716-732): the angle is the host's
        rotate(rc.tilt_cos, op == OP_TILT_NEG ? -rc.tilt_sin : rc.tilt_sin);
    } else if (op == OP_SCALE) {                               // scale_trans (:757-763): a Python float times an S array
        double sc;
        {
#pragma clang fp contract(off)
            sc = rc.scale_lo + (rc.scale_hi - rc.scale_lo) * uniform53();
        }
        const S ss = (S)sc;
#pragma unroll
        for (int dd = 0; dd < 3; ++dd) o[dd] = (float)(ss * x[dd]);
    } else {                                                   // gather / jitter alone
        o[0] = (float)x[0]; o[1] = (float)x[1]; o[2] = (float)x[2];
    }
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- the default recipe as a compile-time specialisation (the kernels' REF = true) ------------------------------------------
// The reference's ten kinds at the reference's strengths, with the list, the slots and the literals folded into the code: the
// chain the kernels had before a recipe could be chosen.  It computes exactly what the table-driven code computes at the
// default recipe (tests/test_gpu_view_recipe.py holds the two to each other bit for bit); it exists because the table-driven
// form measured slower than it at 24 x 2048 out of the resident pool (DESIGN 3.10.1).  The launchers select it when the
// recipe IS the default, strengths included.
static inline bool view_recipe_is_default(const ViewRecipe& rc) {
    const ViewRecipe d = view_recipe_default();
    for (int i = 0; i < d.n; ++i) {
        const ViewPos &a = rc.pos[i], &b = d.pos[i];
        if (a.src != b.src || a.ch != b.ch || a.op != b.op || a.row_slot != b.row_slot || a.row_word != b.row_word ||
            a.jit0 != b.jit0 || a.jit1 != b.jit1 || a.scalar != b.scalar)
            return false;
    }
    return rc.n == d.n && rc.stride == d.stride && rc.sigma == d.sigma &&
           rc.clip == d.clip && rc.rot_range == d.rot_range && rc.scale_lo == d.scale_lo && rc.scale_hi == d.scale_hi &&
           rc.tilt_cos == d.tilt_cos && rc.tilt_sin == d.tilt_sin;
}

__device__ __forceinline__ ViewAt view_at_reference(int G, int chunks) {
    const int c = (int)blockIdx.x % chunks, bv = (int)blockIdx.x / chunks;
    const int v = bv % G;
    return {bv / G, v, v % KINDS, ROUND_SLOTS * (v / KINDS), c * (int)blockDim.x + (int)threadIdx.x};
}

// source of each kind: points 0,0 | key 1,1 | points 0,0 | temporal rows of channel 4, 7 | res1 2 | res2 3
__device__ __forceinline__ int view_source_reference(int k) {
    return k < 2 ? SRC_POINTS : (k < 4 ? SRC_KEY : (k < 6 ? SRC_POINTS : (k < 8 ? SRC_T4 + (k - 6) : k - 6)));
}

__device__ __forceinline__ uint32_t view_row_word_reference(const ViewDraw& q, int k, int slot0, int n) {
    const u32x4 rw = philox4x32_10((uint32_t)n, (uint32_t)(slot0 + (k >> 2)), q.cid, q.epoch, q.k0, q.k1);
    return rw.w[k & 3];
}

struct CosSin { double c, s; };

// The reference's chain: point of view v (kind 0..9) from its source row r (>= 8 channels), one float4 store to dst.  The
// random numbers come from the caller: jz(slot, d) = the CLIPPED jitter np.clip(0.01 z, -0.05, 0.05) of jitter draw `slot`
// (rev 0,1 | ke1 2 | ke2 3,4 | ro1 5 | ro2 6), coordinate d; cossin(k) = cos / sin of the angle of rotation k (views 4, 5).
// Arithmetic follows the reference's dtype walk exactly: jitter in fp64, written back into the S-typed array
// (arr[:, :, :3] = jitter(arr[:, :, :3])), mirror / rotation on a float32 copy, rotation as float32 xyz times an fp64 matrix
// rounded to float32.
template <typename S, class JZ, class CS>
__device__ __forceinline__ void view_chain_reference(const S* __restrict__ r, int v, JZ&& jz, CS&& cossin,
                                                     float* __restrict__ dst) {
    const int c3 = v == 6 ? 4 : (v == 7 ? 7 : 3);            // temporal views: xyz + channel 4 / 7 (:116-117)
    S x[3] = {r[0], r[1], r[2]};
    const S w = r[c3];
    float o[4];
    o[3] = (float)w;
    auto jitter_into_src = [&](int slot) {
#pragma unroll
        for (int d = 0; d < 3; ++d) x[d] = (S)((double)x[d] + jz(slot, d));
    };
    if (v == 1 || v == 3) {                                  // jitter, then reverse_transform (:708-713)
        const int s0 = v == 1 ? 0 : 3;
        jitter_into_src(s0);
        float f[3] = {(float)x[0], (float)x[1], (float)x[2]};
        f[0] = -f[0];
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = (float)((double)f[d] + jz(s0 + 1, d));
    } else if (v == 2) {
        jitter_into_src(2);
        o[0] = (float)x[0]; o[1] = (float)x[1]; o[2] = (float)x[2];
    } else if (v == 4 || v == 5) {                           // jitter, then rotate_trans (:734-749)
        jitter_into_src(v == 4 ? 5 : 6);
        const CosSin a = cossin(v - 4);
        const double fx = (double)(float)x[0], fy = (double)(float)x[1], fz = (double)(float)x[2];
        // [x y z] @ [[c,0,s],[0,1,0],[-s,0,c]]
        o[0] = (float)(fx * a.c + fz * (-a.s));
        o[1] = (float)fy;
        o[2] = (float)(fx * a.s + fz * a.c);
    } else {                                                 // raw, temporal, low-resolution views: plain gather
        o[0] = (float)x[0]; o[1] = (float)x[1]; o[2] = (float)x[2];
    }
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
}

// the chain on Philox draws: point n of a view of kind k in the round whose first slot is slot0
template <typename S>
__device__ __forceinline__ void view_point_reference(const S* __restrict__ r, const ViewDraw& q, int k, int slot0, int n,
                                                     float* __restrict__ dst) {
    view_chain_reference<S>(
        r, k, [&](int slot, int d) { return jit(draw_normal(q, slot0, n, slot, d), 0.01, 0.05); },
        [&](int rot) -> CosSin {
            const double angle = (draw_uniform53(q, slot0 + 24 + rot) - 0.5) * 3.141592653589793 * 0.8;
            return {cos(angle), sin(angle)};
        },
        dst);
}

// ---- the body of the two gather kernels and the tail of their launchers ----------------------------------------------------
// workgroup = one (clip of the batch, view, chunk of up to 512 points); thread = one point.  `from` (by value) says how a
// drawn position becomes a row of src:
//   bool clip(b, first)      go to clip b of the batch; false: it has none (void views; `first` is true in one thread per clip)
//   uint32_t cid()           its dataset index = the Philox counter word
//   int temporal_count(t)    rows of its point cloud whose channel 4 (t = 0) / 7 (t = 1) is non-zero
//   I temporal_row(t, k)     the k-th of them, as a row of src
//   I cloud_row(s, word)     the row of src that `word` draws out of source cloud s (draw_row)
//   channels()               channels per row of src
// idx_out (B, G, P) of I = int32 / int64, optional: the source row of every point, -1 in a void view.  REF: the default
// recipe folded into the code; rc is then unread.
template <typename S, bool REF, class FROM, typename I>
__device__ __forceinline__ void build_view(const S* __restrict__ src, FROM from, int B, int G, int P, int chunks,
                                           int64_t seed, int epoch, float* __restrict__ out, I* __restrict__ idx_out,
                                           const ViewRecipe& rc) {
    const ViewAt at = REF ? view_at_reference(G, chunks) : view_at(rc, G, chunks);
    const int b = at.b, n = at.n;
    if (n >= P) return;                                        // the ragged last chunk of a view
    float* dst = out + (((size_t)at.v * B + b) * P + n) * 4;
    I* io = idx_out ? idx_out + ((size_t)b * G + at.v) * P + n : nullptr;
    if (!from.clip(b, n == 0 && at.v == 0)) {
        view_void(dst);
        if (io) *io = -1;
        return;
    }
    const ViewPos d = REF ? ViewPos{} : rc.pos[at.k];
    const ViewDraw q = view_draw(seed, from.cid(), epoch);
    const int src_of = REF ? view_source_reference(at.k) : (int)d.src;
    const uint32_t word = REF ? view_row_word_reference(q, at.k, at.slot0, n) : view_row_word(q, d, at.slot0, n);
    I row;
    if (src_of >= SRC_T4) {
        const int t = src_of - SRC_T4;
        const int cnt = from.temporal_count(t);
        if (cnt == 0) {                                        // no row to draw from: err is raised, the views are void
            view_void(dst);
            if (io) *io = -1;
            return;
        }
        row = from.temporal_row(t, draw_row(word, cnt));
    } else {
        row = from.cloud_row(src_of, word);
    }
    if (io) *io = row;
    const S* r = src + row * from.channels();
    if (REF) view_point_reference<S>(r, q, at.k, at.slot0, n, dst);
    else view_point<S>(r, q, rc, d, at.slot0, n, dst);
}

// The tail of both launchers.  `own`: the launcher's own refusal (FACL_E_NULL before FACL_E_SHAPE, 0: none); then the shapes
// both refuse, then the alignment of out.  launch(kernel, grid, threads, chunks) starts `ref` when the recipe IS the default,
// strengths included, and `table` otherwise.
template <class K, class L>
static inline int view_launch(int own, K ref, K table, int B, int G, int P, const float* out, const ViewRecipe& rc,
                              L&& launch) {
    if (own != 0) return own;
    if (B < 1 || B > (1 << 20) || !views_gp_ok(G, P)) return FACL_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(out) % 16) return FACL_E_ALIGN;
    const ViewGrid g = view_grid(P);
    launch(view_recipe_is_default(rc) ? ref : table, dim3((unsigned)B * G * g.chunks), dim3(g.threads), g.chunks);
    return facl_launch_status();
}

// the recipe entries: the caller's HOST arrays are checked and turned into the recipe first (no launch on a refusal)
template <class L>
static inline int with_view_recipe(const int32_t* kinds, int n_kinds, const double* strengths, L&& launch) {
    ViewRecipe rc;
    const int e = view_recipe_make(kinds, n_kinds, strengths, &rc);
    return e != 0 ? e : launch(rc);
}

// One pass of the ballot / popcount-prefix walk over rows [c, c + TR_THREADS) of a clip's point cloud (P rows of C
// channels at `cloud`): the rows whose channel 4 / channel 7 is non-zero go, in row order, to l4[run4 + ..] / l7[run7 + ..]
// as `bias + row`; run4 / run7 (uniform across the block) advance by the rows kept.  wtot: 2 x (TR_THREADS / FACL_WAVE)
// ints of shared memory.  Every thread of the block calls it (two barriers inside).
template <typename S, typename R>
__device__ __forceinline__ void temporal_rows_pass(const S* __restrict__ cloud, int C, int P, int c, R bias,
                                                   R* __restrict__ l4, R* __restrict__ l7, int& run4, int& run7,
                                                   int (*wtot)[TR_THREADS / FACL_WAVE]) {
    const int t = threadIdx.x, w = t / FACL_WAVE;
    const unsigned long long below = lanemask_lt();
    const int i = c + t;
    bool nz4 = false, nz7 = false;
    if (i < P) {
        const S* r = cloud + (size_t)i * C;
        nz4 = r[4] != (S)0;
        nz7 = r[7] != (S)0;
    }
    const unsigned long long m4 = __ballot(nz4), m7 = __ballot(nz7);
    if (lane_id() == 0) {
        wtot[0][w] = __popcll(m4);
        wtot[1][w] = __popcll(m7);
    }
    __syncthreads();
    int off4 = run4, off7 = run7, tot4 = 0, tot7 = 0;
#pragma unroll
    for (int k = 0; k < TR_THREADS / FACL_WAVE; ++k) {
        if (k < w) { off4 += wtot[0][k]; off7 += wtot[1][k]; }
        tot4 += wtot[0][k]; tot7 += wtot[1][k];
    }
    if (nz4) l4[off4 + __popcll(m4 & below)] = bias + (R)i;
    if (nz7) l7[off7 + __popcll(m7 & below)] = bias + (R)i;
    run4 += tot4; run7 += tot7;
    __syncthreads();                                          // wtot is rewritten by the next pass
}
