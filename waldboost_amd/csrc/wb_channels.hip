// Fused channel-pyramid kernel for gfx950: one workgroup produces one TU x TV tile of one
// level's final channel image, staging through LDS
//
//   octave base (HBM, uint8/float32)
//     --bilinear, fp64, clip, truncating cast-->   R  : resized tile incl. halo   (LDS, fp32)
//     --Sobel H/D passes, fp64 projection, |.|, 2x2 shrink-->  Sh : shrunk tile  (LDS, float4)
//     --3x3 binomial smooth (fp64 accumulate), zero border-->  channels           (HBM, fp32)
//
// so the resized image, the gradients and the un-smoothed channels never touch HBM.
// Arithmetic follows SURVEY.md S3..S9 operation by operation (compile with
// -ffp-contract=off: no FMA fusion anywhere in this file).
//
// Replaces reference channels.py:127-146 (per-level body of channel_pyramid), :40-52
// (grad_hist), :16-21 (gradients), :55-64 (avg_pool_2), :78-90 (smooth).
//
// This unit: channels_kernel (grad_hist), the projection self-test and the channel stage's C entry points; step 1, the
// tile table and the dispatcher are in wb_chan_tile.h, the other channel functions in wb_chan_u1.hip / wb_chan_gm.hip.
#define WB_CHAN_STAMPS_HERE   // (make STAMPS=1: this unit owns g_chan_stamps)
#include "wb_chan_tile.h"

namespace {

// grad_hist projection of one pixel: out[k] = | fp32( fp64(gx)*cos_k - fp64(gy)*sin_k ) |
// (reference channels.py:47-52)
__device__ inline void project_f64(float gx, float gy, const ChanArgs &a, float *out) {
    double gxd = (double)gx, gyd = (double)gy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float val = (float)(gxd * a.cs[k] - gyd * a.sn[k]);
        out[k] = fmaxf(fabsf(val), 0.0f);
    }
}

// Integer-valued gradients (uint8 images: |g| <= 1020) with the canonical 4-bin constants:
// bit-identical to project_f64 for every (gx, gy) in [-1020, 1020]^2 -- checked exhaustively on
// the device by wb_selftest_projection -- and branch-free:
//   k=0: gx*1 - gy*0 = gx
//   k=2: gx*6.1e-17 - gy rounds to -gy unless gy == 0; then it is fp32(gx * cos(pi/2)), which a
//        two-float split of the constant reproduces
//   k=1,3: the result depends only on d = |gx -/+ gy| (the 1-ulp difference between the fp64 cos
//        and sin of pi/4 is far below fp32 resolution) and fp32(d * sin(pi/4)) equals
//        fma(d, chi, d*clo) for all d <= 2040 -- unless d == 0: then what is left is that 1-ulp
//        difference, |RN64(gx*c1) - RN64(gx*s1)| (0 or one ulp of the product), computed as such.
__device__ inline void project_int(float gx, float gy, const ChanArgs &a, float *out) {
    const float d1 = fabsf(gx - gy), d3 = fabsf(gx + gy), ax = fabsf(gx);
    const double g = (double)gx;
    const float tiny = fabsf((float)(g * a.cs[1] - g * a.sn[1]));
    const float o1 = __builtin_fmaf(d1, a.chi, d1 * a.clo), o3 = __builtin_fmaf(d3, a.chi, d3 * a.clo);
    out[0] = ax;
    out[1] = d1 == 0.0f ? tiny : o1;
    out[2] = gy == 0.0f ? __builtin_fmaf(ax, a.c2hi, ax * a.c2lo) : fabsf(gy);
    out[3] = d3 == 0.0f ? tiny : o3;
}

// project_int without the residues: the four channel values wherever they are "ordinary" (an integer or
// fp32(d*sin(pi/4)) >= 0.7071), and exactly 0 where the reference leaves a ~1e-13 residue (or a true 0).
// Under the 2x2 shrink a residue only shows in the result if every pixel of the block has one (or 0) in
// that channel: fp32 absorbs anything below 3.5e-13 into a value >= 0.7071, in any position of
// ((a+b)+c)+d.  So the shrink is first formed from these values, and only a block whose pooled value
// comes out 0 although it contains a gradient is redone with project_int (channels_kernel, step 2).
// The FAST path runs with the canonical constants only (wb_channels_launch checks), so sin(pi/4) as a two-float split is
// a compile-time constant: literal operands.  (Kernel arguments live in scalar registers, and an fp32 multiply / fmac
// with a scalar-register operand issues in 4 cycles instead of 2 on gfx950 -- tools/valu_class_probe.hip.)  The split
// product is odd in d, so it is formed from the signed difference and the |.| is left to the consumer's source modifier.
constexpr float kSinHi = 0x1.6a09e6p-1f;
constexpr float kSinLo = (float)(0x1.6a09e667f3bccp-1 - (double)kSinHi);
__device__ inline void project_ordinary(float gx, float gy, const ChanArgs &, float *out) {
    // (every result opaque to the SLP vectoriser: paired into v_pk_* the operations cost more issue cycles than plain ones,
    // and a packed instruction takes no |x| modifier -- eight v_and per shrunk pixel materialised the absolute values)
    const float d1 = gx - gy, d3 = gx + gy;
    out[0] = fabsf(gx);
    out[1] = fabsf(scalar_only(__builtin_fmaf(d1, kSinHi, scalar_only(d1 * kSinLo))));
    out[2] = fabsf(gy);
    out[3] = fabsf(scalar_only(__builtin_fmaf(d3, kSinHi, scalar_only(d3 * kSinLo))));
}

// (launch bound: 4 workgroups = 4 waves per SIMD is what the 39 KB of LDS of a float R admit; without it the register
// allocator may trade that occupancy for a few more registers -- measured: 138 VGPRs, 3 waves per SIMD, +17 % time.
// Shrink 2 on uint8 images with the smooth -- the detection path -- is held to five: 26 KB of LDS, <= 96 VGPRs.
// Shrink 4 on uint8 images: five as well, what the 31 KB of LDS of a byte R admit)
constexpr int kChanS4Waves = 5;
template <typename T, int S, int TU, int TV, bool SMOOTH, bool FAST, int NT>
__global__ __launch_bounds__(NT, sizeof(T) == 8 ? 1
                                 : S == 4  ? (sizeof(T) == 1 ? kChanS4Waves : 1)
                                 : (S == 2 && sizeof(T) == 1 && SMOOTH && FAST) ? 5
                                                                               : 4) void channels_kernel(ChanArgs a) {
    using G = TileGeom<S, TU, TV, SMOOTH, NT>;
    constexpr int HS = G::HS, SV = G::SV, RH = G::RH, RW = G::RW, P = G::P;
    constexpr int PATCH_BYTES = sizeof(T) == 1 ? G::PATCH_BYTES : 0;
    constexpr int UNI_MIN = G::SH_BYTES > PATCH_BYTES ? G::SH_BYTES : PATCH_BYTES;
    // uint8 images at shrink 2 and 4: R holds the resized pixels as BYTES (they are integers 0..255) -- a quarter of the LDS,
    // and the rank tables no longer fit in R: they go to `uni`.
    // Shrink 4: 5.9 KB instead of 23 KB, the tables parked behind the shrunk tile (the dead source patch): 31 KB of LDS per
    // workgroup = five per CU instead of three, which a latency-bound kernel wants (three kept the vector ALUs 42 % busy);
    // the price is one conversion per R store and 36 per shrunk pixel's patch read.
    // Shrink 2 (round 5): 5.2 KB instead of 20.4 KB; the tables do not fit behind the 19 KB shrunk tile, so they go OVER it,
    // once every thread has read its Sh values (one more barrier): 26 KB of LDS instead of 40 KB per workgroup.
    constexpr bool RBYTES = sizeof(T) == 1 && S != 1;
    constexpr bool LUT_OVER_SH = RBYTES && S == 2;
    constexpr int UNI_LUT = !RBYTES ? 0 : LUT_OVER_SH ? WB_BIN16_LUT_BYTES : ((G::SH_BYTES + 15) & ~15) + WB_BIN16_LUT_BYTES;
    constexpr int UNI_BYTES = UNI_MIN > UNI_LUT ? UNI_MIN : UNI_LUT;
    using RT = typename std::conditional<RBYTES, uint8_t, float>::type;
    constexpr int RP = RPitch<RT, RW>::value;
    constexpr bool LUT_IN_UNI = RBYTES;
    // (the tables of either width: WB_BIN16_LUT_BYTES is the larger)
    static_assert(WB_BIN16_LUT_BYTES >= WB_BIN_LUT_BYTES, "table sizes");
    constexpr int R_BYTES = LUT_IN_UNI ? RH * RP : (RH * RW * 4 > WB_BIN16_LUT_BYTES ? RH * RW * 4 : WB_BIN16_LUT_BYTES);   // (float R later holds the rank tables)
    __shared__ __attribute__((aligned(16))) unsigned char Rraw[R_BYTES];
    RT *R = reinterpret_cast<RT *>(Rraw);
    __shared__ __attribute__((aligned(16))) unsigned char uni[UNI_BYTES];
    unsigned char *lut_lds = LUT_OVER_SH ? uni : LUT_IN_UNI ? uni + ((G::SH_BYTES + 15) & ~15) : Rraw;
    __shared__ uint32_t odd_values;      // set when a shrunk value lies outside the exact-sum range (see step 3)
    __shared__ float4 rowtab[sizeof(T) == 1 ? RH + RW % 64 : 1];   // row taps of the tile, taps of the RW % 64 last columns (uint8 images, staged patch)
    F4 *Sh = reinterpret_cast<F4 *>(uni);
    constexpr bool SEPARABLE = SMOOTH && FAST;
    if (SEPARABLE && threadIdx.x == 0) odd_values = 0;

    const WbTile tile = a.tiles[blockIdx.x];
    const WbLevel L = a.levels[tile.level];
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int u0 = tile.ty * TU, v0 = tile.tx * TV;

    const T *src = (L.oct == 0) ? (const T *)a.img + (int64_t)b * a.img_stride
                                : (const T *)a.oct + (int64_t)b * a.oct_stride + L.src_off;
    double mn, mx;
    clip_range<T>(a, b, L.oct, mn, mx);

    const int ry0 = S * (u0 - HS) - 1, rx0 = S * (v0 - HS) - 1;
    // a tile on the bottom edge of its level holds fewer than TU output rows: the shrunk rows (su_need) and resized
    // rows (rh_need) behind them are all the steps below compute (7 % of the tiles' rows at 1080p lie past an edge)
    const int vrows = L.u - u0 < TU ? L.u - u0 : TU;
    const int su_need = vrows + 2 * HS, rh_need = S * su_need + 2;
    WB_CSTAMP(0);
    resample_tile<T, G, false, RT, RBYTES && S == 2>(a, L, src, mn, mx, ry0, rx0, rh_need, R, uni, rowtab, tid);
    __syncthreads();
    WB_CSTAMP(4);
    if (a.dbg & 1) return;

    // ---- step 2: gradients -> 4 oriented channels -> shrink, one shrunk pixel per call
    //      Rp: the pixel's (S + 2) x (S + 2) patch of R, Shp: where its shrunk value goes
    //      grads: where the gradients come from -- OwnPatch{}: the pixel reads its patch (at ro) and forms them itself; else a
    //      callable that hands them over (the row runs below, which carry half of every patch from the pixel above);
    //      everything behind the gradients is the same code for both
    struct OwnPatch {};
    auto shrunk_pixel = [&](const int ro, const int so, auto grads) {     // (offsets, not pointers: R's alignment stays visible -- 8-byte reads)
        float ch[S][S][4], gxs[S][S], gys[S][S];
        constexpr bool TWO_PASS = FAST && S > 1;          // ordinary values first, residues only where they can show
        if constexpr (!std::is_same<decltype(grads), OwnPatch>::value) {
            grads(gxs, gys);
        } else if constexpr (RBYTES && S == 2) {
            // The 4 x 4 patch starts at the even column 2j of a dword-padded row: a patch row is two aligned 16-bit reads
            // (volatile: never merged into one dword read at a 2-byte boundary, which LDS serves slowly) and four byte
            // conversions.  The gradients are then formed differences first -- the centre row / column of a [-1,0,1] pass
            // has weight 0 -- and [1,2,1] pass second: on pixels 0..255 every partial sum is an integer of magnitude <= 1020,
            // exact in fp32 in either order, so gx and gy are the values the passes below give (zeros included: +0 both ways).
            float pt[P][P];
#pragma unroll
            for (int y = 0; y < P; ++y) {
                const uint32_t lo = lds_u16_vol(Rraw, ro + y * RP), hi = lds_u16_vol(Rraw, ro + y * RP + 2);
                pt[y][0] = (float)(lo & 0xffu);
                pt[y][1] = (float)(lo >> 8);
                pt[y][2] = (float)(hi & 0xffu);
                pt[y][3] = (float)(hi >> 8);
            }
            float ex[P][S], dy[S][P];     // column differences (for gx), row differences (for gy)
#pragma unroll
            for (int r = 0; r < P; ++r)
#pragma unroll
                for (int x = 0; x < S; ++x) ex[r][x] = scalar_only(pt[r][x] - pt[r][x + 2]);
#pragma unroll
            for (int y = 0; y < S; ++y)
#pragma unroll
                for (int c = 0; c < P; ++c) dy[y][c] = scalar_only(pt[y][c] - pt[y + 2][c]);
#pragma unroll
            for (int y = 0; y < S; ++y)
#pragma unroll
                for (int x = 0; x < S; ++x) {
                    gxs[y][x] = scalar_only(Src<T>::hpass(ex[y][x], ex[y + 1][x], ex[y + 2][x]));
                    gys[y][x] = scalar_only(Src<T>::hpass(dy[y][x], dy[y][x + 1], dy[y][x + 2]));
                }
        } else {
        float pt[P][P];
        if constexpr (RBYTES) {
            // six bytes per patch row = two aligned dwords (the patch starts at column S * j = 4 j of a dword-padded row)
            static_assert(P == 6 && RP % 4 == 0, "shrink-4 patch rows");
#pragma unroll
            for (int y = 0; y < P; ++y) {
                const uint32_t *w = reinterpret_cast<const uint32_t *>(R + ro + y * RP);
                const uint32_t w0 = w[0], w1 = w[1];
                pt[y][0] = (float)(w0 & 0xffu);
                pt[y][1] = (float)((w0 >> 8) & 0xffu);
                pt[y][2] = (float)((w0 >> 16) & 0xffu);
                pt[y][3] = (float)(w0 >> 24);
                pt[y][4] = (float)(w1 & 0xffu);
                pt[y][5] = (float)((w1 >> 8) & 0xffu);
            }
        } else {
#pragma unroll
            for (int y = 0; y < P; ++y)
#pragma unroll
                for (int x = 0; x < P; ++x) pt[y][x] = R[ro + y * RP + x];
        }

        float hc[S][P];   // vertical [1,2,1] pass at patch rows 1..S
        float hr[P][S];   // horizontal [1,2,1] pass at patch cols 1..S
#pragma unroll
        for (int y = 0; y < S; ++y)
#pragma unroll
            for (int x = 0; x < P; ++x) hc[y][x] = scalar_only(Src<T>::hpass(pt[y][x], pt[y + 1][x], pt[y + 2][x]));
#pragma unroll
        for (int y = 0; y < P; ++y)
#pragma unroll
            for (int x = 0; x < S; ++x) hr[y][x] = scalar_only(Src<T>::hpass(pt[y][x], pt[y][x + 1], pt[y][x + 2]));

#pragma unroll
        for (int y = 0; y < S; ++y)
#pragma unroll
            for (int x = 0; x < S; ++x) {
                gxs[y][x] = scalar_only(Src<T>::dpass(hc[y][x], hc[y][x + 1], hc[y][x + 2]));
                gys[y][x] = scalar_only(Src<T>::dpass(hr[y][x], hr[y + 1][x], hr[y + 2][x]));
            }
        }
#pragma unroll
        for (int y = 0; y < S; ++y)
#pragma unroll
            for (int x = 0; x < S; ++x) {
                const float gx = gxs[y][x], gy = gys[y][x];
                if constexpr (TWO_PASS)
                    project_ordinary(gx, gy, a, ch[y][x]);
                else if constexpr (FAST)
                    project_int(gx, gy, a, ch[y][x]);
                else
                    project_f64(gx, gy, a, ch[y][x]);
            }

        float o[4];
        auto pool = [&]() {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (S == 1) {
                    o[k] = ch[0][0][k];
                } else if constexpr (S == 2) {
                    o[k] = scalar_only(scalar_only(scalar_only(scalar_only(ch[0][0][k] + ch[1][0][k]) + ch[0][1][k]) + ch[1][1][k]) * 0.25f);
                } else {  // S == 4 (extension): avg_pool_2 applied twice
                    float q[2][2];
#pragma unroll
                    for (int A = 0; A < 2; ++A)
#pragma unroll
                        for (int B = 0; B < 2; ++B)
                            q[A][B] = scalar_only(scalar_only(scalar_only(scalar_only(ch[2 * A][2 * B][k] + ch[2 * A + 1][2 * B][k]) +
                                                                  ch[2 * A][2 * B + 1][k]) + ch[2 * A + 1][2 * B + 1][k]) * 0.25f);
                    o[k] = scalar_only(scalar_only(scalar_only(scalar_only(q[0][0] + q[1][0]) + q[0][1]) + q[1][1]) * 0.25f);
                }
            }
        };
        // integer gradients: a shrunk value is 0, or in [0.17, 1443] (some pixel of the block had an
        // ordinary value), or a sum of the 1e-13-sized residues of the projection -- the smooth wants to
        // know about the last kind (step 3)
        auto flag_odd = [&]() {
            const uint32_t lo = __float_as_uint(0.125f) - 1u;
            const uint32_t m01 = min(__float_as_uint(o[0]) - 1u, __float_as_uint(o[1]) - 1u);
            const uint32_t m23 = min(__float_as_uint(o[2]) - 1u, __float_as_uint(o[3]) - 1u);
            if (min(m01, m23) < lo) odd_values = 1;
        };
        pool();
        if constexpr (TWO_PASS) {
            // a pooled 0 in a block that has a gradient (pooled |gx| != 0): every pixel of the block holds a
            // residue or 0 in that channel -- rare; redo the block with the exact values
            if (o[0] != 0.0f && fminf(fminf(o[1], o[2]), o[3]) == 0.0f) {
#pragma unroll
                for (int y = 0; y < S; ++y)
#pragma unroll
                    for (int x = 0; x < S; ++x) project_int(gxs[y][x], gys[y][x], a, ch[y][x]);
                pool();
                if constexpr (SEPARABLE) flag_odd();
            }
        } else if constexpr (SEPARABLE) {
            flag_odd();
        }
        Sh[so] = F4{o[0], o[1], o[2], o[3]};
    };
    // Tiles whose shrunk width is a wave or a little more (the 16 x 64 tiles: 66 columns): a wave owns whole rows, lane =
    // column, so a pixel's LDS addresses are the previous round's plus a constant (no division by the width, no 64-bit
    // multiply-add per pixel: round 4); the few columns beyond the 64th go to the last wave, which owns the fewest rows
    // (one stand-alone pixel each).
    constexpr bool ROWMAP = SV >= 64 && SV - 64 <= 8 && NT % 64 == 0;
    if constexpr (ROWMAP) {
        constexpr int NWV = NT / 64, XC = SV - 64;
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        if constexpr (RBYTES && S == 2) {
            // Round 7: a wave owns CONTIGUOUS rows -- su_need rows over the waves as evenly as they go, the longer runs
            // first (18 rows: 5, 5, 4, 4; the last wave, with the extra columns below, still owns the fewest) --, because
            // the patch of the pixel below is this pixel's patch moved down two rows: of its four patch rows two are
            // already in registers.  What is carried is not the converted bytes but what the gradients take from them,
            // per patch row r: the column differences ex[r][x] = pt[r][x] - pt[r][x + 2] (gx = their vertical [1,2,1]
            // pass, as in the stand-alone pixel) and the horizontal [1,2,1] sums hr[r][x] = pt[r][x] + 2 pt[r][x + 1] +
            // pt[r][x + 2], of which gy is the row difference hr[y][x] - hr[y + 2][x]: the [1,2,1] pass first and the
            // [-1,0,1] pass second, where the stand-alone pixel has them the other way round.  On pixels 0..255 every
            // partial sum of either order is an integer of magnitude <= 1020, exact in fp32, so both give the same bits
            // (a zero is +0 both ways: x - x and an exact fma sum of 0 are +0 under round-to-nearest).
            // A row after a wave's first then reads two patch rows instead of four (4 LDS halfwords, 8 conversions) and
            // needs 24 instead of 32 plain operations.  Unrolled completely, with a wave-uniform exit: nothing is carried
            // around a back edge (round 4), the carried values are renamed, not moved.  A bottom-edge tile (su_need from
            // 3) may leave a wave without a row.
            constexpr int MAXR = (G::SU + NWV - 1) / NWV;
            const int q = su_need / NWV, rem = su_need % NWV;
            const int n_w = q + (wave < rem ? 1 : 0), i_w = wave * q + (wave < rem ? wave : rem);
            const int ro = S * (i_w * RP + lane), so = i_w * SV + lane;
            // (the conversions opaque: left visible, the compiler does the differences and sums on the bytes as integers and
            // converts each of them -- six conversions per patch row instead of four)
            auto patch_row = [&](const uint32_t lo, const uint32_t hi, float (&e)[S], float (&h)[S]) {
                const float p0 = scalar_only((float)(lo & 0xffu)), p1 = scalar_only((float)(lo >> 8));
                const float p2 = scalar_only((float)(hi & 0xffu)), p3 = scalar_only((float)(hi >> 8));
                e[0] = scalar_only(p0 - p2);
                e[1] = scalar_only(p1 - p3);
                h[0] = scalar_only(Src<T>::hpass(p0, p1, p2));
                h[1] = scalar_only(Src<T>::hpass(p1, p2, p3));
            };
            float ex[P][S], hr[P][S];
#pragma unroll
            for (int r = 0; r < MAXR; ++r) {
                if (r >= n_w) break;                                                  // wave-uniform
                const int o = ro + r * S * RP;
                // the patch rows that are new to this pixel (all four for a wave's first): every read before the arithmetic
                const int y0 = r == 0 ? 0 : S;
                uint32_t lo[P], hi[P];
#pragma unroll
                for (int y = 0; y < P; ++y) {
                    if (y < y0) continue;
                    lo[y] = lds_u16_vol(Rraw, o + y * RP);
                    hi[y] = lds_u16_vol(Rraw, o + y * RP + 2);
                }
#pragma unroll
                for (int y = 0; y < P; ++y) {
                    if (y >= y0) {
                        patch_row(lo[y], hi[y], ex[y], hr[y]);
                    } else {
#pragma unroll
                        for (int x = 0; x < S; ++x) {
                            ex[y][x] = ex[y + S][x];
                            hr[y][x] = hr[y + S][x];
                        }
                    }
                }
                shrunk_pixel(o, so + r * SV, [&](float (&gxs)[S][S], float (&gys)[S][S]) {
#pragma unroll
                    for (int y = 0; y < S; ++y)
#pragma unroll
                        for (int x = 0; x < S; ++x) {
                            gxs[y][x] = scalar_only(Src<T>::hpass(ex[y][x], ex[y + 1][x], ex[y + 2][x]));
                            gys[y][x] = scalar_only(hr[y][x] - hr[y + 2][x]);
                        }
                });
            }
        } else {
            int ro = S * (wave * RP + lane), so = wave * SV + lane;
#pragma nounroll
            for (int i = wave; i < su_need; i += NWV) {                           // wave-uniform trip count
                shrunk_pixel(ro, so, OwnPatch{});
                ro += NWV * S * RP;
                so += NWV * SV;
            }
        }
        if constexpr (XC > 0) {
            if (wave == NWV - 1) {
                for (int p = lane; p < su_need * XC; p += 64) {
                    const int i = p / XC, j = 64 + p - i * XC;
                    shrunk_pixel(S * (i * RP + j), i * SV + j, OwnPatch{});
                }
            }
        }
    } else {
        for (int p = tid; p < su_need * SV; p += NT) {
            const int i = p / SV, j = p - i * SV;
            shrunk_pixel(S * (i * RP + j), p, OwnPatch{});
        }
    }
    // rank tables of the model (12 KiB, L2-resident): requested before the barrier, parked in R -- dead once every
    // thread has left step 2 -- right behind it (float R), behind the shrunk tile (shrink 4, byte R), or over the shrunk
    // tile once the smooth has read it (shrink 2, byte R: the loads are in flight across the smooth)
    constexpr int LUT_VECS = WB_BIN_LUT_BYTES / 16, LUT16_VECS = WB_BIN16_LUT_BYTES / 16;
    auto ranks_wide_tag = [](const ChanArgs &aa) { return aa.rank != nullptr && aa.rank_wide != 0; };
    static_assert(LUT_VECS == 768 && NT == 256, "three vectors per thread");
    const bool ranks = a.rank != nullptr;
    uint4 lut0 = make_uint4(0, 0, 0, 0), lut1 = lut0, lut2 = lut0, lut3 = lut0, lut4 = lut0;
    const bool wide_lut = ranks_wide_tag(a);
    if (ranks) {
        lut0 = a.rank_lut[tid];
        lut1 = a.rank_lut[tid + 256];
        lut2 = a.rank_lut[tid + 512];
        if (wide_lut && !LUT_OVER_SH) {                       // (the 16-bit tables: 1280 vectors)
            lut3 = a.rank_lut[tid + 768];
            lut4 = a.rank_lut[tid + 1024];
        }
    }
    static_assert(LUT16_VECS == 1280, "five vectors per thread");
    auto park_tables = [&]() {
        uint4 *lut = reinterpret_cast<uint4 *>(lut_lds);
        lut[tid] = lut0;
        lut[tid + 256] = lut1;
        lut[tid + 512] = lut2;
        if (wide_lut) {
            if constexpr (LUT_OVER_SH) {                      // (requested only here: 8 registers fewer across the smooth)
                lut3 = a.rank_lut[tid + 768];
                lut4 = a.rank_lut[tid + 1024];
            }
            lut[tid + 768] = lut3;
            lut[tid + 1024] = lut4;
        }
    };
    __syncthreads();
    if (!LUT_OVER_SH && ranks) park_tables();
    WB_CSTAMP(5);

    if (a.dbg & 2) return;
    // ---- step 3: 3x3 binomial smooth (fp64 sum in source order, /16, one rounding), border = 0.
    //      Each thread owns RPT vertically adjacent outputs of one column, so every shrunk value
    //      it needs is read and widened to fp64 once for up to three output rows.
    // (tiles that do not split into whole strips -- 8 x 30 on 256 threads: one output per thread, the last threads idle)
    constexpr bool WHOLE = TU * TV % NT == 0 && NT % TV == 0;
    constexpr int RPT = WHOLE ? TU * TV / NT : 1;
    static_assert(WHOLE || TU * TV <= NT, "one output per thread");
    float *out = reinterpret_cast<float *>(a.chn) + (int64_t)b * a.chn_stride + L.chn_off;
    const int j = tid % TV, i0 = (tid / TV) * RPT;
    const int sv = v0 + j;
    float o[RPT][4];
    // (64-wide tiles: a wave owns whole output rows, so on a bottom-edge tile the waves whose rows lie past the level
    // skip the smooth and the ranks -- wave-uniform; they still meet the barrier below)
    const bool live = WHOLE ? (TV != 64 || u0 + __builtin_amdgcn_readfirstlane(i0) < L.u) : i0 < TU;
#pragma unroll
    for (int y = 0; y < RPT; ++y) o[y][0] = o[y][1] = o[y][2] = o[y][3] = 0.0f;
    if (!live) {
    } else if constexpr (SMOOTH) {
        if (SEPARABLE && odd_values == 0) {
            // Every value of the tile is 0 or a float32 in [2^-3, 2^11): all partial sums of the nine
            // weighted terms are multiples of 2^-26 below 2^15 -- exact in fp64 in ANY order.  So the
            // row sums are formed once, row by row, and shared by the three output rows that use them.
            // Channels 0 and 2 -- |gx| and |gy| of integer gradients, pooled -- are multiples of 2^-2 (2^-4 under the
            // shrink-4 extension) below 2^10: their nine-term sums have at most 18 significant bits and are exact in
            // fp32 too, so these two channels need neither the conversions nor the fp64 arithmetic (the fp64 sum is the
            // same real number, /16 is exact, and the result is representable: identical bits).
            double s[3][2];
            float s32[3][2];
#pragma unroll
            for (int y = 0; y < RPT + 2; ++y) {
                const F4 c0 = Sh[(i0 + y) * SV + j], c1 = Sh[(i0 + y) * SV + j + 1], c2 = Sh[(i0 + y) * SV + j + 2];
                const float a0[4] = {c0.x, c0.y, c0.z, c0.w}, a1[4] = {c1.x, c1.y, c1.z, c1.w}, a2[4] = {c2.x, c2.y, c2.z, c2.w};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    s32[y % 3][h] = __builtin_fmaf(2.0f, a1[2 * h], a0[2 * h]) + a2[2 * h];
                    s[y % 3][h] = __builtin_fma(2.0, (double)a1[2 * h + 1], (double)a0[2 * h + 1]) + (double)a2[2 * h + 1];
                }
                if (y >= 2) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        o[y - 2][2 * h] = (__builtin_fmaf(2.0f, s32[(y - 1) % 3][h], s32[(y - 2) % 3][h]) + s32[y % 3][h]) * 0.0625f;
                        o[y - 2][2 * h + 1] = (float)((__builtin_fma(2.0, s[(y - 1) % 3][h], s[(y - 2) % 3][h]) + s[y % 3][h]) * 0.0625);
                    }
                }
            }
        } else {
            // the rows streamed: each output's chain takes its three rows in order (smooth9 row by row), so a row is widened
            // once, used by the up to three outputs whose window holds it, and dropped -- the tile's 72 widened values are
            // never live at once (with the rank tables in flight across the smooth they did not fit the registers; the
            // scheduling barrier keeps the compiler from hoisting every row's reads to the top again)
            double s[RPT][4];
#pragma unroll
            for (int r = 0; r < RPT + 2; ++r) {
                __builtin_amdgcn_sched_barrier(0);
                const F4 c0 = Sh[(i0 + r) * SV + j], c1 = Sh[(i0 + r) * SV + j + 1], c2 = Sh[(i0 + r) * SV + j + 2];
                const float a0[4] = {c0.x, c0.y, c0.z, c0.w}, a1[4] = {c1.x, c1.y, c1.z, c1.w}, a2[4] = {c2.x, c2.y, c2.z, c2.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double v0 = a0[k], v1 = a1[k], v2 = a2[k];
                    if (r >= 2) o[r - 2][k] = smooth_bot(s[r - 2][k], v0, v1, v2);
                    if (r >= 1 && r - 1 < RPT) s[r - 1][k] = smooth_mid(s[r - 1][k], v0, v1, v2);
                    if (r < RPT) s[r][k] = smooth_top(v0, v1, v2);
                }
            }
        }
    } else {
#pragma unroll
        for (int y = 0; y < RPT; ++y) {
            F4 c = Sh[(i0 + y) * SV + j];
            o[y][0] = c.x; o[y][1] = c.y; o[y][2] = c.z; o[y][3] = c.w;
        }
    }
    if (LUT_OVER_SH && ranks) {
        __syncthreads();                                      // every thread holds its Sh values: the tables go over them
        park_tables();
    }
    WB_CSTAMP(6);
#pragma unroll
    for (int y = 0; y < RPT; ++y) {
        const int su = u0 + i0 + y;
        if ((!WHOLE && !live) || su >= L.u || sv >= L.v || (a.dbg & 4)) continue;
        if (SMOOTH && (su == 0 || sv == 0 || su == L.u - 1 || sv == L.v - 1)) o[y][0] = o[y][1] = o[y][2] = o[y][3] = 0.0f;
        // one float4 per pixel ([u][v][4]): 64 lanes store 1 KiB contiguous
        if (a.chn) {
            float4 *dst = reinterpret_cast<float4 *>(out + ((int64_t)su * L.v + sv) * 4);
            *dst = make_float4(o[y][0], o[y][1], o[y][2], o[y][3]);
        }
    }
    if (ranks) {
        // the same pixels as threshold ranks, one dword per pixel -- or, 16-bit ranks, eight bytes (wb_common.h: wb_bin_rank)
        __syncthreads();                                      // the tables are in LDS
        const float *Sthr = reinterpret_cast<const float *>(lut_lds);
        const int K = a.rank_iters;
        auto rank_pixels = [&](auto wide_tag) {
            constexpr bool WIDE = decltype(wide_tag)::value;
            constexpr int SLOTS = WIDE ? WB_BIN16_SLOTS : WB_BIN_SLOTS, CELLS = WIDE ? WB_BIN16_CELLS : WB_BIN_CELLS;
            const uint8_t *base8 = reinterpret_cast<const uint8_t *>(lut_lds) + 4 * SLOTS * 4;
            const uint16_t *base16 = reinterpret_cast<const uint16_t *>(base8);
            // all RPT x 4 values of the thread advance together: every step is RPT * 4 independent LDS lookups (one
            // value at a time, the 1 + K dependent lookups of each value were a chain of LDS latencies)
            uint32_t r[RPT][4];
            if (live) {
#pragma unroll
                for (int y = 0; y < RPT; ++y)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t cell = wb_bin_cell(o[y][k], a.rank_k[k], a.rank_b[k], (float)(CELLS - 1));
                        r[y][k] = WIDE ? (uint32_t)base16[k * CELLS + cell] : (uint32_t)base8[k * CELLS + cell];
                    }
                if (K <= 2) {
                    // the usual case -- at most two thresholds share a cell: both candidates S[r], S[r + 1] come with ONE
                    // LDS read (they are neighbours) and are compared independently: S is sorted, so the second test only
                    // passes where the first does; a threshold of a higher cell, or the +inf padding, never passes
                    // (r + 1 <= the table's last padding slot stays inside the channel's table)
#pragma unroll
                    for (int y = 0; y < RPT; ++y)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float *sp = Sthr + k * SLOTS + r[y][k];
                            const float s0 = sp[0], s1 = sp[1];
                            r[y][k] += (o[y][k] > s0 ? 1u : 0u) + (o[y][k] > s1 ? 1u : 0u);
                        }
                } else if (WIDE && K <= 4) {
                    // the coarser 16-bit grid: up to four thresholds per cell, all four candidates S[r .. r + 3] fetched at
                    // once (r + 3 <= 1023: the table's last four slots are +inf padding)
#pragma unroll
                    for (int y = 0; y < RPT; ++y)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float *sp = Sthr + k * SLOTS + r[y][k];
                            const float s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
                            r[y][k] += (o[y][k] > s0 ? 1u : 0u) + (o[y][k] > s1 ? 1u : 0u) + (o[y][k] > s2 ? 1u : 0u) + (o[y][k] > s3 ? 1u : 0u);
                        }
                } else {
                    for (int i = 0; i < K; ++i) {
#pragma unroll
                        for (int y = 0; y < RPT; ++y)
#pragma unroll
                            for (int k = 0; k < 4; ++k) r[y][k] += o[y][k] > Sthr[k * SLOTS + r[y][k]] ? 1u : 0u;
                    }
                }
            }
#pragma unroll
            for (int y = 0; y < RPT; ++y) {
                const int su = u0 + i0 + y;
                if (!live || su >= L.u || sv >= L.v || (a.dbg & 4)) continue;
                uint32_t rk[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    rk[k] = r[y][k];
                    if constexpr (sizeof(T) != 1) rk[k] = o[y][k] != o[y][k] ? (WIDE ? 65535u : 255u) : rk[k];   // a NaN pixel fails every `v <= thr`
                }
                if constexpr (WIDE) {
                    uint2 *rout = reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(a.rank) + ((int64_t)b * a.rank_stride + L.chn_off));
                    rout[(int64_t)su * L.v + sv] = make_uint2(rk[0] | (rk[1] << 16), rk[2] | (rk[3] << 16));
                } else {
                    uint32_t *rout = reinterpret_cast<uint32_t *>(a.rank + (int64_t)b * a.rank_stride + L.chn_off);
                    rout[(int64_t)su * L.v + sv] = rk[0] | (rk[1] << 8) | (rk[2] << 16) | (rk[3] << 24);
                }
            }
        };
        if (a.rank_wide)
            rank_pixels(std::true_type{});
        else
            rank_pixels(std::false_type{});
    }
    WB_CSTAMP(7);
}

// Exhaustive device check of project_int against project_f64 over [-1020, 1020]^2.
__global__ void selftest_projection_kernel(ChanArgs a, uint32_t *mismatches) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = 2041;
    if (i >= n * n) return;
    float gx = (float)(i / n - 1020), gy = (float)(i % n - 1020);
    float f[4], r[4];
    project_int(gx, gy, a, f);
    project_f64(gx, gy, a, r);
    for (int k = 0; k < 4; ++k)
        if (__float_as_uint(f[k]) != __float_as_uint(r[k])) atomicAdd(mismatches, 1u);
}

// T: how the image is held; FAST: integer gradients with the canonical constants (project_int / project_ordinary)
template <typename T, bool FAST>
int launch_hist(hipStream_t st, dim3 grid, const ChanArgs &a, int shrink, bool smooth) {
    // diagnostic (WB_CHAN_XLDS=bytes): extra dynamic LDS per workgroup lowers the workgroups per CU, to tell a
    // latency-bound kernel (time ~ 1 / residency) from a throughput-bound one (time unchanged)
    static const size_t xlds = getenv("WB_CHAN_XLDS") ? (size_t)atoi(getenv("WB_CHAN_XLDS")) : 0;
    return chan_dispatch("wb_channels_launch", shrink, smooth, [&](auto s, auto sm) {
        constexpr int S = decltype(s)::value;
        constexpr ChanTile t = chan_tile(WB_CHN_GRAD_HIST, S);
        hipLaunchKernelGGL((channels_kernel<T, S, t.tu, t.tv, decltype(sm)::value, FAST, t.nt>), grid, dim3(t.nt), xlds, st, a);
        WB_HIP_CHECK(hipGetLastError());
        return WB_OK;
    });
}

// the canonical constants np.cos/np.sin(np.linspace(0, pi, 5)[:-1]) the integer fast path is proven for
const double kCanonCs[4] = {1.0, 0x1.6a09e667f3bcdp-1, 0x1.1a62633145c07p-54, -0x1.6a09e667f3bccp-1};
const double kCanonSn[4] = {0.0, 0x1.6a09e667f3bccp-1, 1.0, 0x1.6a09e667f3bcdp-1};

bool canonical_constants(const double *cs_sn) {
    for (int k = 0; k < 4; ++k)
        if (cs_sn[k] != kCanonCs[k] || cs_sn[4 + k] != kCanonSn[k]) return false;
    return true;
}

void set_constants(ChanArgs &a, const double *cs_sn) {
    for (int k = 0; k < 4; ++k) {
        a.cs[k] = cs_sn[k];
        a.sn[k] = cs_sn[4 + k];
    }
    a.chi = (float)cs_sn[5];
    a.clo = (float)(cs_sn[5] - (double)a.chi);
    a.c2hi = (float)cs_sn[2];
    a.c2lo = (float)(cs_sn[2] - (double)a.c2hi);
}

}  // namespace

extern "C" int wb_channels_tile(int channel_func, int shrink, int *tile_u, int *tile_v) {
    WB_REQUIRE(tile_u && tile_v, "wb_channels_tile: null pointer");
    return chan_dispatch("wb_channels_tile", shrink, false, [&](auto s, auto) {
        const ChanTile t = chan_tile(channel_func, decltype(s)::value);
        *tile_u = t.tu;
        *tile_v = t.tv;
        return WB_OK;
    });
}

extern "C" int wb_channel_func_info(int channel_func, int *n_channels, int *chn_dtype) {
    WB_REQUIRE(n_channels && chn_dtype, "wb_channel_func_info: null pointer");
    switch (channel_func) {
        case WB_CHN_GRAD_HIST: *n_channels = 4; *chn_dtype = WB_DTYPE_F32; return WB_OK;
        case WB_CHN_GRAD_HIST_4_U1: *n_channels = 4; *chn_dtype = WB_DTYPE_U8; return WB_OK;
        case WB_CHN_GRAD_MAG_U1: *n_channels = 1; *chn_dtype = WB_DTYPE_U8; return WB_OK;
        case WB_CHN_GRAD_MAG: *n_channels = 1; *chn_dtype = WB_DTYPE_F32; return WB_OK;
    }
    wb_set_error("wb_channel_func_info: unknown channel function %d", channel_func);
    return WB_ERR_INVALID;
}

// Per tile, the source patch it stages (WbTilePatch): the kernels' own extent function, on the host, with the geometry of
// the kernel that channel_func / shrink / smooth select.
namespace {
template <typename G, bool FULL_ROWS>
void fill_patches(const WbLevel *levels, const WbTile *tiles, int n_tiles, WbTilePatch *out) {
    for (int i = 0; i < n_tiles; ++i) {
        const WbTile &t = tiles[i];
        const WbLevel &L = levels[t.level];
        const int u0 = t.ty * G::TU, v0 = t.tx * G::TV;
        const int ry0 = G::S * (u0 - G::HS) - 1, rx0 = G::S * (v0 - G::HS) - 1;
        // (channels_kernel computes only the rows a tile on the bottom edge of its level needs; the uint8 kernels all RH)
        const int vrows = L.u - u0 < G::TU ? L.u - u0 : G::TU;
        const int rh = FULL_ROWS ? G::RH : G::S * (vrows + 2 * G::HS) + 2;
        int r_lo, c_lo, nrow, nbyte;
        const bool staged = tile_patch_extent<G, false>(L, ry0, rx0, rh, r_lo, c_lo, nrow, nbyte);
        WbTilePatch &o = out[i];
        o.r_lo = staged ? r_lo : 0;
        o.c_lo = staged ? c_lo : 0;
        o.rows = staged ? (uint16_t)nrow : 0;
        o.bytes = staged ? (uint16_t)nbyte : 0;
        o.pad = 0;
    }
}
template <int FUNC>
int fill_patches_for(int shrink, bool smooth, const WbLevel *levels, const WbTile *tiles, int n_tiles, WbTilePatch *out) {
    return chan_dispatch("wb_channels_tile_patches", shrink, smooth, [&](auto s, auto sm) {
        constexpr int S = decltype(s)::value;
        constexpr ChanTile t = chan_tile(FUNC, S);
        fill_patches<TileGeom<S, t.tu, t.tv, decltype(sm)::value, t.nt>, FUNC != WB_CHN_GRAD_HIST>(levels, tiles, n_tiles, out);
        return WB_OK;
    });
}
}  // namespace

extern "C" int wb_channels_tile_patches(int channel_func, int shrink, int smooth, const WbLevel *levels_host, int n_levels,
                                        const WbTile *tiles_host, int n_tiles, WbTilePatch *out_host) {
    WB_REQUIRE(levels_host && tiles_host && out_host && n_levels >= 1 && n_tiles >= 0, "wb_channels_tile_patches: null pointer / empty plan");
    for (int i = 0; i < n_tiles; ++i)
        WB_REQUIRE(tiles_host[i].level >= 0 && tiles_host[i].level < n_levels, "wb_channels_tile_patches: tile %d names level %d of %d", i,
                   tiles_host[i].level, n_levels);
    switch (channel_func) {
        case WB_CHN_GRAD_HIST: return fill_patches_for<WB_CHN_GRAD_HIST>(shrink, smooth != 0, levels_host, tiles_host, n_tiles, out_host);
        case WB_CHN_GRAD_HIST_4_U1: return fill_patches_for<WB_CHN_GRAD_HIST_4_U1>(shrink, smooth != 0, levels_host, tiles_host, n_tiles, out_host);
        case WB_CHN_GRAD_MAG_U1: return fill_patches_for<WB_CHN_GRAD_MAG_U1>(shrink, smooth != 0, levels_host, tiles_host, n_tiles, out_host);
    }
    wb_set_error("wb_channels_tile_patches: channel function %d takes no patch table", channel_func);
    return WB_ERR_UNSUPPORTED;
}

extern "C" int wb_channels_launch(void *stream, const void *img, int64_t img_stride, const void *oct,
                                  int64_t oct_stride, int dtype, int batch, const WbLevel *levels,
                                  int n_levels, const WbTile *tiles, int n_tiles, const uint32_t *minmax,
                                  int n_oct, const WbTap *taps, int channel_func, int shrink, int smooth,
                                  const double *cs_sn, void *chn, int64_t chn_stride, const WbModel *rank_model,
                                  uint8_t *rank, int64_t rank_stride) {
    return wb_channels_launch_x(stream, img, img_stride, oct, oct_stride, dtype, batch, levels, n_levels, tiles, n_tiles, minmax,
                                n_oct, taps, channel_func, shrink, smooth, cs_sn, chn, chn_stride, rank_model, rank, rank_stride,
                                nullptr, WB_DTYPE_RANK8);
}

extern "C" int wb_channels_launch_x(void *stream, const void *img, int64_t img_stride, const void *oct,
                                    int64_t oct_stride, int dtype, int batch, const WbLevel *levels,
                                    int n_levels, const WbTile *tiles, int n_tiles, const uint32_t *minmax,
                                    int n_oct, const WbTap *taps, int channel_func, int shrink, int smooth,
                                    const double *cs_sn, void *chn, int64_t chn_stride, const WbModel *rank_model,
                                    uint8_t *rank, int64_t rank_stride, const WbTilePatch *patches, int rank_dtype) {
    WB_REQUIRE(img && levels && tiles && minmax && taps && (chn || rank), "wb_channels_launch: null pointer");
    WB_REQUIRE(!rank == !rank_model, "wb_channels_launch: rank and rank_model go together");
    WB_REQUIRE(!rank || rank_dtype == WB_DTYPE_RANK8 || rank_dtype == WB_DTYPE_RANK16, "wb_channels_launch_x: rank_dtype %d (WB_DTYPE_RANK8 or WB_DTYPE_RANK16)", rank_dtype);
    const int rank_form = rank ? wb_tile_form(rank_dtype) : -1;
    const bool wide = rank_form == WB_FORM_RANK16;
    WB_REQUIRE(!wide || rank_model->form[WB_FORM_RANK16].present, "wb_channels_launch_x: this model has no 16-bit rank tables (wb_model_info: rank16_ok)");
    WB_REQUIRE(!wide || wb_aligned(rank, 8), "wb_channels_launch_x: 16-bit ranks must be 8-byte aligned");
    WB_REQUIRE(!patches || (dtype == WB_DTYPE_U8 && channel_func != WB_CHN_GRAD_MAG),
               "wb_channels_launch_x: the patch table goes with uint8 images and the gradient-histogram kernels");
    WB_REQUIRE(!rank || channel_func == WB_CHN_GRAD_HIST, "wb_channels_launch: ranks are written for grad_hist channels only");
    WB_REQUIRE(!rank || wide || rank_model->form[WB_FORM_RANK8].present, "wb_channels_launch: this model has no rank tables (wb_model_info: rank_ok)");
    WB_REQUIRE(!rank || wb_aligned(rank, 4), "wb_channels_launch: rank must be 4-byte aligned");
    WB_REQUIRE(cs_sn || channel_func != WB_CHN_GRAD_HIST, "wb_channels_launch: grad_hist needs the orientation constants");
    WB_REQUIRE(batch >= 1 && n_levels >= 1 && n_tiles >= 1, "wb_channels_launch: empty launch");
    WB_REQUIRE(batch <= 65535, "wb_channels_launch: batch %d exceeds grid.y limit", batch);
    WB_REQUIRE(smooth == 0 || smooth == 1, "wb_channels_launch: smooth must be 0 or 1");
    WB_REQUIRE(n_oct >= 1 && n_oct <= WB_MAX_OCTAVES, "wb_channels_launch: n_oct out of range");
    ChanArgs a;
    a.img = img;
    a.oct = oct;
    a.img_stride = img_stride;
    a.oct_stride = oct_stride;
    a.levels = levels;
    a.tiles = tiles;
    a.minmax = minmax;
    a.taps = taps;
    a.n_oct = n_oct;
    a.chn = chn;
    a.chn_stride = chn_stride;
    a.src_int = 0;
    a.rank = rank;
    a.rank_stride = rank_stride;
    a.rank_lut = nullptr;
    a.rank_iters = 0;
    a.patches = patches;
    a.rank_wide = wide ? 1 : 0;
    if (rank) {
        const WbRankTable &rt = wb_rank_table(rank_model, rank_form);
        a.rank_lut = reinterpret_cast<const uint4 *>(rt.lut_dev);
        a.rank_iters = rt.iters;
        for (int k = 0; k < 4; ++k) {
            a.rank_k[k] = rt.k[k];
            a.rank_b[k] = rt.b[k];
        }
    }
    if (cs_sn) set_constants(a, cs_sn);
    static const int dbg = getenv("WB_CHAN_DBG") ? atoi(getenv("WB_CHAN_DBG")) : 0;
    a.dbg = dbg;
    dim3 grid((unsigned)n_tiles, (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (channel_func == WB_CHN_GRAD_HIST_4_U1 || channel_func == WB_CHN_GRAD_MAG_U1) {
        if (dtype != WB_DTYPE_U8) {
            wb_set_error("wb_channels_launch: the uint8 channel functions take uint8 images (8 bit input, fpga/channels.py:32)");
            return WB_ERR_UNSUPPORTED;
        }
        return wb_chan_launch_u1(st, grid, &a, channel_func, shrink, smooth != 0);
    }
    if (channel_func == WB_CHN_GRAD_MAG) {
        // H = (1,2,..,6,..,2,1) as float32, divided by its float32 sum (channels.py:11-13)
        for (int i = 0; i < 11; ++i) a.tri[i] = (double)((float)(i < 6 ? i + 1 : 11 - i) / 36.0f);
        a.gm_eps = 1e-3f;
        return wb_chan_launch_gm(st, grid, &a, dtype, shrink, smooth != 0);
    }
    if (channel_func != WB_CHN_GRAD_HIST) {
        wb_set_error("wb_channels_launch: channel function %d has no kernel", channel_func);
        return WB_ERR_UNSUPPORTED;
    }
    if (dtype == WB_DTYPE_U8) {
        // integer gradients + canonical constants: exact fp32 projection (see project_int)
        static const bool no_fast = getenv("WB_CHAN_NO_FAST") != nullptr;
        if (canonical_constants(cs_sn) && !no_fast) return launch_hist<uint8_t, true>(st, grid, a, shrink, smooth != 0);
        return launch_hist<uint8_t, false>(st, grid, a, shrink, smooth != 0);
    }
    if (dtype == WB_DTYPE_F32) return launch_hist<float, false>(st, grid, a, shrink, smooth != 0);
    if (wb_dtype_held_f64(dtype)) {
        a.src_int = wb_cast_mode(dtype);
        return launch_hist<double, false>(st, grid, a, shrink, smooth != 0);
    }
    wb_set_error("wb_channels_launch: unsupported image dtype code %d", dtype);
    return WB_ERR_UNSUPPORTED;
}

extern "C" int wb_selftest_projection(void *stream, uint32_t *mismatches) {
    WB_REQUIRE(mismatches, "wb_selftest_projection: null pointer");
    ChanArgs a = {};
    double cs_sn[8];
    for (int k = 0; k < 4; ++k) {
        cs_sn[k] = kCanonCs[k];
        cs_sn[4 + k] = kCanonSn[k];
    }
    set_constants(a, cs_sn);
    const int n = 2041 * 2041;
    hipLaunchKernelGGL(selftest_projection_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, mismatches);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

#ifdef WB_CASC_STAMPS
#include <vector>
// Diagnostic build: mean microseconds between consecutive stamps over the first n_wg workgroups of
// the last channel launch (s_memrealtime ticks at 100 MHz).  Workgroups that skipped a phase
// (direct path) contribute 0 to it.
extern "C" int wb_debug_channel_stamps(int n_wg, double *mean_us7, double *lifetime_us) {
    if (n_wg > WB_CSTAMP_WGS) n_wg = WB_CSTAMP_WGS;
    std::vector<unsigned long long> h((size_t)n_wg * WB_CSTAMP_SLOTS);
    WB_HIP_CHECK(hipDeviceSynchronize());
    WB_HIP_CHECK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_chan_stamps), h.size() * 8));
    double acc[7] = {0}, life = 0;
    for (int w = 0; w < n_wg; ++w) {
        const unsigned long long *s = &h[(size_t)w * WB_CSTAMP_SLOTS];
        for (int k = 0; k < 7; ++k) acc[k] += (double)(s[k + 1] - s[k]);
        life += (double)(s[7] - s[0]);
    }
    for (int k = 0; k < 7; ++k) mean_us7[k] = acc[k] / n_wg / 100.0;
    *lifetime_us = life / n_wg / 100.0;
    return WB_OK;
}
#endif
