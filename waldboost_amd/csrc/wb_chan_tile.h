// What the channel kernels share: arguments, source-dtype traits, the tile geometry with its ONE table of output tiles,
// step 1 of every tile kernel (resample_tile) and the host's shrink x smooth dispatcher.  The units:
//   wb_channels.hip     grad_hist (channels_kernel), the self-test, the C entry points
//   wb_chan_u1.hip      grad_hist_4_u1 / grad_mag_u1 (channels_u1_kernel)
//   wb_chan_gm.hip      grad_mag (channels_gm_kernel)
//   wb_chan_levels.hip  the plain per-level kernels (resize_level / pool2 / smooth)       (all in the anonymous namespace)
#pragma once
#include <stdlib.h>
#include <type_traits>

#include "wb_common.h"

// launchers of the units without a C entry point (chan_args: a ChanArgs, whose type is private to each unit)
int wb_chan_launch_u1(hipStream_t st, dim3 grid, const void *chan_args, int channel_func, int shrink, bool smooth);
int wb_chan_launch_gm(hipStream_t st, dim3 grid, const void *chan_args, int dtype, int shrink, bool smooth);

namespace {

struct ChanArgs {
    const void *img;
    const void *oct;
    int64_t img_stride, oct_stride;
    const WbLevel *levels;
    const WbTile *tiles;
    const uint32_t *minmax;
    const WbTap *taps;
    int n_oct;
    void *chn;           // [u][v][C] per level, dtype of the channel function
    int64_t chn_stride;
    double cs[4], sn[4];
    float chi, clo;      // sin(pi/4) = chi + clo (two-float split) for the integer-gradient fast path
    float c2hi, c2lo;    // cos(pi/2) (fp64: 6.1e-17) likewise
    double tri[11];      // grad_mag: triangle_kernel(5) (float32 values, widened)
    float gm_eps;        // grad_mag: float32(1e-3)
    int src_int;         // float64-held image dtypes: how the resize result is cast back (WB_CAST_*: .astype(image dtype))
    int dbg;             // diagnostics (WB_CHAN_DBG): 1 = stop after step 1, 2 = after step 2, 4 = skip the stores
    // optional second output of channels_kernel: the pixels as threshold ranks of one model (WB_DTYPE_RANK8)
    uint8_t *rank;       // [u][v][4] bytes per level, same element offsets as chn; nullptr = none
    int64_t rank_stride;
    const WbTilePatch *patches;   // optional (uint8 images): per tile, the source patch it stages (wb_channels_tile_patches)
    const uint4 *rank_lut;   // WbRankTable::lut_dev: float S[4][256], then uint8 base[4][WB_BIN_CELLS]
    int rank_iters;
    float rank_k[4], rank_b[4];
    int rank_wide;       // 0: WB_DTYPE_RANK8 (one dword per pixel), 1: WB_DTYPE_RANK16 (uint16 x 4 = 8 bytes per pixel; WB_BIN16_* tables)
};

// Diagnostic build only (make STAMPS=1): thread 0 of every workgroup stores s_memrealtime at the
// phase boundaries into a private slot; wb_debug_channel_stamps turns them into mean wall-clock per
// phase.  Never part of a measured build.  Only the unit that reads the array back (wb_channels.hip) defines it and stamps.
#if defined(WB_CASC_STAMPS) && defined(WB_CHAN_STAMPS_HERE)
#define WB_CSTAMP_SLOTS 8
#define WB_CSTAMP_WGS (1 << 17)
__device__ unsigned long long g_chan_stamps[WB_CSTAMP_WGS * WB_CSTAMP_SLOTS];
#define WB_CSTAMP(k)                                                                                      \
    do {                                                                                                  \
        unsigned long long _wg = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;                 \
        if (threadIdx.x == 0 && _wg < WB_CSTAMP_WGS)                                                      \
            g_chan_stamps[_wg * WB_CSTAMP_SLOTS + (k)] = __builtin_amdgcn_s_memrealtime();                \
    } while (0)
#else
#define WB_CSTAMP(k) do {} while (0)
#endif

typedef WbTap Tap;   // one axis of the bilinear resample (scipy NI_ZoomShift, order 1), host-built table

// a double held by lane `k` (wave-uniform k), to every lane
__device__ inline double lane_f64(double v, int k) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// A byte from LDS that is never merged with its neighbour's: two adjacent byte loads otherwise become ONE 16-bit load at an
// arbitrary (odd) address, and unaligned LDS accesses are slow on gfx950 (measured: -3.7 % on the whole kernel with the
// pairs kept apart).  A VOLATILE load through an LDS (address space 3) pointer: no flat_load, and a constant displacement
// still folds into the instruction's offset field -- the four tap bytes of a pixel (i0, i0 + 1 in two consecutive patch
// rows) come from ONE address register.
typedef const volatile __attribute__((address_space(3))) unsigned char *LdsVolBytePtr;
__device__ __forceinline__ uint8_t lds_byte_vol(const unsigned char *patch, int off) {
    return *((LdsVolBytePtr)patch + off);
}
// ... and two bytes at an even offset (one aligned ds_read_u16; volatile for the same reason: never merged with the next pair)
typedef const volatile __attribute__((address_space(3))) uint16_t *LdsVolU16Ptr;
__device__ __forceinline__ uint32_t lds_u16_vol(const unsigned char *base, int off) {
    return *(LdsVolU16Ptr)((LdsVolBytePtr)base + off);
}

// scipy's order-1 resample of one output pixel: fp64, taps and additions in NI_ZoomShift's order
__device__ inline double resample_f64(double v00, double v01, double v10, double v11, const Tap &tr, const Tap &tc) {
    double t = (v00 * tr.w0) * tc.w0;
    t = t + (v01 * tr.w0) * tc.w1;
    t = t + (v10 * tr.w1) * tc.w0;
    t = t + (v11 * tr.w1) * tc.w1;
    return t;
}

template <typename T> struct Src;
template <> struct Src<uint8_t> {
    static constexpr bool kFastResample = true;
    // The uint8 result is floor(clip(t)), so only the integer part of t matters.  An fp32 estimate
    // (4 bytes x weights rounded to fp32, fma chain) is within 1.1e-4 of the exact sum, and scipy's
    // fp64 value within 1e-12: unless the estimate lies within EPS of an integer both have the same
    // floor.  Lanes inside that band (flat 2x2 patches always are) redo the pixel in fp64.
    static constexpr float kEps = 2.5e-4f;
    // No clip here: outside the band the exact value lies strictly between two integers of
    // [min, max] (it is a convex combination of pixels of the octave), so its floor is in range.
    static __device__ bool fast(float v00, float v01, float v10, float v11, float wr0, float wr1, float wc0, float wc1,
                                float &out) {
        float top = __builtin_fmaf(v01, wc1, v00 * wc0), bot = __builtin_fmaf(v11, wc1, v10 * wc0);
        return fast_rows(top, bot, wr0, wr1, out);
    }
    // the same from the two rows' horizontal interpolations (a row's value is shared by the output rows that tap it)
    static __device__ bool fast_rows(float top, float bot, float wr0, float wr1, float &out) {
        // (opaque to the SLP vectoriser: paired into v_pk_mul / v_pk_fma / v_pk_add the two rows of a pass cost more issue
        // cycles than as plain fp32 instructions)
        float t = hold(__builtin_fmaf(bot, wr1, hold(top * wr0)));
        float fl = floorf(t), fr = hold(t - fl);
        out = fl;
        return fabsf(hold(fr - 0.5f)) <= 0.5f - kEps;
    }
    static __device__ __forceinline__ float hold(float v) {
        asm volatile("" : "+v"(v));
        return v;
    }
    static __device__ double lo(uint32_t k) { return (double)k; }
    // fp64 result is clipped in fp64, then cast to uint8 by truncation
    static __device__ float finish(double t, double mn, double mx, int) {
        t = fmin(fmax(t, mn), mx);
        return (float)(int)t;
    }
    static __device__ bool taps_finite(uint8_t, uint8_t, uint8_t) { return true; }
    // [1,2,1] pass: exact in fp32 for integer pixels (|.| <= 1020); 2b is exact, so the fma rounds like b*2 + (a+c)
    static __device__ float hpass(float a, float b, float c) { return __builtin_fmaf(b, 2.0f, a + c); }
    // [-1,0,1] pass: scipy multiplies the centre tap too (weight 0); integer pixels are finite, so it adds nothing
    static __device__ float dpass(float lo, float, float hi) { return lo - hi; }
};
template <> struct Src<float> {
    static constexpr bool kFastResample = false;
    static __device__ bool fast(float, float, float, float, float, float, float, float, float &) { return false; }
    static __device__ bool fast_rows(float, float, float, float, float &) { return false; }
    static __device__ double lo(uint32_t k) { return (double)wb_key_f32(k); }
    // float32 images: zoom stores fp32, then np.clip in fp32 -- np.minimum(np.maximum(x, lo), hi), which hands a NaN
    // through from x AND from a bound: an octave that holds a NaN pixel has a NaN min or max (wb_octaves.hip: the
    // keys order NaNs outside +-inf) and every pixel resized from it is NaN, as under NumPy
    static __device__ float finish(double t, double mn, double mx, int) {
        const float f = (float)t, lo = (float)mn, hi = (float)mx;
        if (lo != lo || hi != hi) return __builtin_nanf("");
        return f < lo ? lo : (f > hi ? hi : f);              // (a NaN f fails both tests and stays)
    }
    // a pixel copy stands for scipy's (v00*1)*1 + (v01*1)*0 + (v10*0)*1 + (v11*0)*0 only while the three taps of
    // weight 0 are finite (0 * inf = NaN)
    static __device__ bool taps_finite(float a, float b, float c) { return fabsf(a) < INFINITY && fabsf(b) < INFINITY && fabsf(c) < INFINITY; }
    // scipy correlate1d: fp64 accumulate, one fp32 rounding per pass
    static __device__ float hpass(float a, float b, float c) {
        return (float)((double)b * 2.0 + ((double)a + (double)c));
    }
    // the centre tap of weight 0 is part of the sum (correlate1d's antisymmetric branch): 0 * inf = NaN next to an
    // infinite value, as under scipy; for a finite centre it adds +-0
    static __device__ float dpass(float lo, float mid, float hi) { return (float)((double)mid * 0.0 + ((double)lo - (double)hi)); }
};

// float64 images, and integer images held as float64 (WB_DTYPE_F64 / WB_DTYPE_I8..U32): zoom in fp64, np.clip in
// fp64 to the octave's range, .astype(image dtype) -- truncation toward zero for the integer types -- and then the
// channel function's own astype("f") (reference channels.py:132, :41).  Gradients as for float32 images.
template <> struct Src<double> {
    static constexpr bool kFastResample = false;
    static __device__ bool fast(float, float, float, float, float, float, float, float, float &) { return false; }
    static __device__ bool fast_rows(float, float, float, float, float &) { return false; }
    static __device__ double lo(unsigned long long k) {
        const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
        return __longlong_as_double((long long)b);
    }
    static __device__ float finish(double t, double mn, double mx, int src_int) {
        if (mn != mn || mx != mx) return __builtin_nanf("");     // (np.clip with a NaN bound: see Src<float>::finish)
        t = t < mn ? mn : (t > mx ? mx : t);
        switch (src_int) {
            case WB_CAST_TRUNC: t = trunc(t) + 0.0; break;      // (+ 0.0: trunc(-0.5) is -0.0, the integer types have one zero)
            case WB_CAST_BOOL: t = t != 0.0 ? 1.0 : 0.0; break;
            case WB_CAST_F16: t = wb_round_f16(t); break;
        }
        return (float)t;
    }
    static __device__ bool taps_finite(double a, double b, double c) { return fabs(a) < INFINITY && fabs(b) < INFINITY && fabs(c) < INFINITY; }
    static __device__ float hpass(float a, float b, float c) { return Src<float>::hpass(a, b, c); }
    static __device__ float dpass(float lo, float mid, float hi) { return Src<float>::dpass(lo, mid, hi); }
};

// the (min, max) an octave's resize result is clipped to, from the order-preserving keys the octave kernel left
// (32-bit keys for uint8 / float32 images, 64-bit ones for the float64-held dtypes; word 0 holds max(~key))
template <typename T> __device__ inline void clip_range(const ChanArgs &a, int b, int oct, double &mn, double &mx) {
    if constexpr (sizeof(T) == 8) {
        const unsigned long long *mm = reinterpret_cast<const unsigned long long *>(a.minmax) + ((int64_t)b * a.n_oct + oct) * 2;
        mn = Src<T>::lo(~mm[0]);
        mx = Src<T>::lo(mm[1]);
    } else {
        const uint32_t *mm = a.minmax + ((int64_t)b * a.n_oct + oct) * 2;
        mn = Src<T>::lo(~mm[0]);
        mx = Src<T>::lo(mm[1]);
    }
}

struct F4 {
    float x, y, z, w;
};

// Opaque to the optimiser: stops the SLP vectoriser from pairing neighbouring scalar fp32 operations into
// v_pk_* instructions -- on gfx950 a packed op issues in 4 cycles against 2 for each scalar op, and building
// its operand pairs costs extra v_movs (tools/valu_rate_probe.hip)
__device__ inline float scalar_only(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// reference channels.py:78-83: nine-term sum in source order; numba promotes int64*float32 to
// fp64, so the sum is fp64; "/16" and one rounding to fp32 on the store.
// 2*x and 4*x are exact, so fma(2, b, acc) rounds exactly like acc + 2*b: same bits, half the ops.
// The chain row by row (the top, middle and bottom row's three terms), for callers that stream the rows.
__device__ inline double smooth_top(double a, double b, double c) { return __builtin_fma(2.0, b, a) + c; }
__device__ inline double smooth_mid(double s, double d, double e, double f) {
    return __builtin_fma(2.0, f, __builtin_fma(4.0, e, __builtin_fma(2.0, d, s)));
}
__device__ inline float smooth_bot(double s, double g, double h, double i) { return (float)((__builtin_fma(2.0, h, s + g) + i) * 0.0625); }
__device__ inline float smooth9(double a, double b, double c, double d, double e, double f, double g, double h, double i) {
    return smooth_bot(smooth_mid(smooth_top(a, b, c), d, e, f), g, h, i);
}

// Tile geometry shared by the channel kernels: TU x TV outputs per workgroup of NT threads, shrink S
template <int S_, int TU_, int TV_, bool SMOOTH_, int NT_ = 256> struct TileGeom {
    static constexpr int S = S_, TU = TU_, TV = TV_, NT = NT_, NW = NT_ / 64;
    static constexpr bool SMOOTH = SMOOTH_;
    static constexpr int HS = SMOOTH ? 1 : 0;
    static constexpr int SU = TU + 2 * HS, SV = TV + 2 * HS;  // shrunk tile incl. smooth halo
    static constexpr int RH = S * SU + 2, RW = S * SV + 2;    // resized tile incl. the 3x3 gradient halo
    static constexpr int P = S + 2;                           // patch side per shrunk pixel
    // LDS: R (resized tile) | one region shared by the uint8 source patch (live in step 1 only)
    // and the shrunk tile Sh (live from step 2 on).  Source patch capacity: no larger than a
    // float4 Sh, so that R + region stay under 40 KiB (4 workgroups per CU); tiles of the most
    // down-scaled levels of an octave that do not fit take the direct path
    // (shrink 2: 74 rows x 256 bytes instead of 80 x 236 -- the most down-scaled level of an octave of 8, zoom step
    // 1.834, needs 72 rows of 254 bytes and took the direct path before)
    // (shrink 4, an extension: 42 x 138 resized pixels per 8 x 32 outputs tap up to 86 source rows of 278 bytes -- five
    // times the shrunk tile, so the patch gets its own size; sized after the shrunk tile no shrink-4 tile was ever staged)
    static constexpr int PROWS = S == 2 ? (TU == 16 ? 74 : 2 * RH - 8) : 2 * RH + 4;
    static constexpr int PPITCH = S == 4 ? 2 * RW + 12 : (S == 2 && TU != 16) ? 256 : ((SU * SV * 16) / PROWS) & ~3;
    static_assert(S == 4 || PROWS * PPITCH <= SU * SV * 16, "the source patch shares the shrunk tile's memory");
    static_assert(PPITCH % 4 == 0, "patch rows are written as dwords");
    static constexpr int SH_BYTES = SU * SV * 16;
    static constexpr int PATCH_BYTES = PROWS * PPITCH;
};

// ---- step 1 of every channel kernel: bilinear resample of the tile (+ 1-pixel gradient halo) into
//      R, cast back to the image dtype.
//      One tile row per wave at a time: the row's taps are wave-uniform (scalar registers,
//      scalar row base pointers), the column taps of a lane's NCS columns live in registers,
//      and the 4*NCS source loads of a row are issued before any arithmetic.  Coordinates are
//      clamped to the level = the 'reflect' halo of convolve1d for a 1-pixel border.
//      The RW % 64 right-most columns are done afterwards, one pixel per thread.
//      Ends without a barrier: the caller synchronises before reading R.
__host__ __device__ inline int reflect_index(int i, int n) {      // scipy 'reflect': (d c b a | a b c d | d c b a)
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i >= n ? period - 1 - i : i;
}

// Coordinate i of a tile (possibly outside its level of n pixels) -> the level pixel it stands for: clamped (= the
// 'reflect' halo of a 1-pixel border: the gradient kernels) or reflected (grad_mag's 6-pixel halo).
template <bool REFLECT> __host__ __device__ __forceinline__ int tile_coord(int i, int n) {
    if constexpr (REFLECT)
        return reflect_index(i, n);
    else
        return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// ... and bounds [lo_out, hi_out] on the level pixels the coordinates lo..hi stand for (conservative under reflection:
// they only size the staged source patch).
template <bool REFLECT> __host__ __device__ __forceinline__ void tile_coord_range(int lo, int hi, int n, int &lo_out, int &hi_out) {
    if constexpr (!REFLECT) {
        lo_out = tile_coord<false>(lo, n);
        hi_out = tile_coord<false>(hi, n);
    } else if (lo >= 0 && hi < n) {
        lo_out = lo;
        hi_out = hi;
    } else if (lo < -n || hi >= 2 * n || (lo < 0 && hi >= n)) {
        lo_out = 0;
        hi_out = n - 1;
    } else if (lo < 0) {                                  // mirrored at the top / left edge: -1 - i
        lo_out = hi < 0 ? -1 - hi : 0;
        hi_out = hi < 0 ? -1 - lo : (hi > -1 - lo ? hi : -1 - lo);
    } else {                                              // mirrored at the bottom / right edge: 2n - 1 - i
        hi_out = lo >= n ? 2 * n - 1 - lo : n - 1;
        lo_out = lo >= n ? 2 * n - 1 - hi : (lo < 2 * n - 1 - hi ? lo : 2 * n - 1 - hi);
    }
}

// The source patch a uint8 tile stages: rows r_lo .. r_lo + nrow - 1, bytes c_lo .. c_lo + nbyte - 1 of the level's octave,
// for tile rows ry0 .. ry0 + rh - 1 and columns rx0 .. rx0 + RW - 1; false when the tile does not stage one.  Strict
// down-scale on both axes: every tap pair is (i0, i0 + 1), no mirroring (plan.axis_taps), and the extents follow from the
// first and last coordinate's i0 = floor((k + 0.5) * step - 0.5) -- the host's own fp64 expression for the tap table.
// The SAME function runs on the host (wb_channels_tile_patches: IEEE fp64 on both sides, no contraction) and, without a
// table, in every workgroup.
template <typename G, bool REFLECT>
__host__ __device__ __forceinline__ bool tile_patch_extent(const WbLevel &L, int ry0, int rx0, int rh, int &r_lo, int &c_lo, int &nrow,
                                                           int &nbyte) {
    int yf, yl, xf, xl;
    tile_coord_range<REFLECT>(ry0, ry0 + rh - 1, L.nh, yf, yl);
    tile_coord_range<REFLECT>(rx0, rx0 + G::RW - 1, L.nw, xf, xl);
    const bool ident = (L.src_h == L.nh) && (L.src_w == L.nw);
    const bool strict = !ident && L.src_h > L.nh && L.src_w > L.nw;
    auto first_tap = [](int k, double step) { return (int)floor(((double)k + 0.5) * step - 0.5); };
    r_lo = first_tap(yf, L.sy);
    c_lo = first_tap(xf, L.sx);
    const int r_hi = first_tap(yl, L.sy) + 1, c_hi = first_tap(xl, L.sx) + 1;
    nrow = r_hi - r_lo + 1;
    nbyte = c_hi - c_lo + 1;
    return strict && nrow + 1 <= G::PROWS && nbyte + 8 <= G::PPITCH;
}

// RT: how R holds a resized pixel -- float, or (uint8 images only: the pixels are integers 0..255) one byte, rows padded to
// whole dwords: a quarter of the LDS, for the price of one conversion per store here and one per read in the caller.
template <typename RT, int RW> struct RPitch { static constexpr int value = sizeof(RT) == 1 ? ((RW + 3) & ~3) : RW; };

// Settled by measurement: patch rows a wave has in flight while it stages the source patch, rows per pass of the resample
constexpr int kChanUR = 8, kChanRB = 2;
// rows of a wave's strip of the resample: an even share of the rh tile rows, rounded up to whole passes of kChanRB rows --
// 42 rows on four waves are then 12 + 12 + 12 + 6 (21 passes) instead of 11 + 11 + 11 + 9 (23: each ended on a pass of one)
__host__ __device__ constexpr int wb_strip_rows(int rh, int nw) { return kChanRB * ((rh + nw * kChanRB - 1) / (nw * kChanRB)); }

template <typename T, typename G, bool REFLECT = false, typename RT = float, bool RADD = false>
__device__ __forceinline__ void resample_tile(const ChanArgs &a, const WbLevel &L, const T *src, const double mn,
                                              const double mx, const int ry0, const int rx0, const int rh, RT *R,
                                              unsigned char *uni, float4 *rowtab, const int tid) {
    static_assert(sizeof(RT) == 4 || sizeof(T) == 1, "byte R holds uint8 pixels");
    constexpr int RP = RPitch<RT, G::RW>::value;             // R's row pitch in elements
    // (RADD -- byte R at shrink 2, round 7: v is an integer of [0, 255] on every path -- the fast path's floor lies in the octave's
    // range, the redo is clipped and truncated, the identity path copies a byte -- so v + 2^23 is exact and the low byte
    // of its bits IS that integer: one add of the fast issue class instead of a conversion of the slow one, the same byte
    // store.  Opaque to the SLP vectoriser like the arithmetic around it.)
    auto rput = [&](int idx, float v) {
        if constexpr (sizeof(RT) == 1 && RADD)
            R[idx] = (RT)__float_as_uint(scalar_only(v + 8388608.0f));
        else if constexpr (sizeof(RT) == 1)
            R[idx] = (RT)(int)v;
        else
            R[idx] = v;
    };
    // rh <= RH: the tile rows that are needed (a tile on the bottom edge of its level uses fewer): wave-uniform, the
    // strips below are cut from it
    constexpr int RH = G::RH, RW = G::RW, PPITCH = G::PPITCH, NT = G::NT, NW = G::NW;
    const Tap *__restrict__ rtap = a.taps + L.tap_off;      // row taps [nh], then column taps [nw]
    const Tap *__restrict__ ctap = rtap + L.nh;
    constexpr int NCS = RW / 64, MAINW = NCS * 64, LEFT = RW - MAINW;
    // (readfirstlane: the wave index is the same in every lane -- said explicitly, the row loops below run on
    // scalar counters and branches instead of vector compares and exec masks)
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Levels at their octave's own size (scale 1: every level i=0 with even dims) resample with
    // weights (1, 0): t = v*1*1 + 0 + 0 + 0 = v exactly -> plain copy.
    const bool ident = (L.src_h == L.nh) && (L.src_w == L.nw);
    if constexpr (sizeof(T) == 1) {
        // ... and for a tile that lies inside the level (no clamped coordinate) the copy is done four pixels at a time: one
        // (unaligned) dword load, four byte conversions, two 8-byte LDS stores -- every load of the tile in flight at
        // once, no taps.  One level in eight is such a level and it is the largest of its octave (21 % of all tiles).
        constexpr int RWD = (RW + 3) / 4;
        if (ident && ry0 >= 0 && ry0 + RH <= L.nh && rx0 >= 0 && rx0 + 4 * RWD <= L.nw) {
            static_assert(RW % 2 == 0, "pixel pairs");
            typedef uint32_t __attribute__((aligned(1))) u32u;
            constexpr int NE = RH * RWD, PER = (NE + NT - 1) / NT;
            uint32_t v[PER];
            int at[PER];
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                int e = tid + NT * i;
                e = e < NE ? e : NE - 1;                              // (duplicates rewrite the same values)
                const int k = e / RWD, d = e - k * RWD;
                v[i] = *reinterpret_cast<const u32u *>(src + (int64_t)(ry0 + k) * L.src_w + rx0 + 4 * d);
                at[i] = k * RP + 4 * d;
            }
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if constexpr (sizeof(RT) == 1) {
                    *reinterpret_cast<uint32_t *>(R + at[i]) = v[i];        // (the source bytes ARE the pixels; rows are whole dwords)
                } else {
                    float2 *dst = reinterpret_cast<float2 *>(R + at[i]);
                    dst[0] = make_float2((float)(v[i] & 0xffu), (float)((v[i] >> 8) & 0xffu));
                    if (at[i] % RW + 2 < RW) dst[1] = make_float2((float)((v[i] >> 16) & 0xffu), (float)(v[i] >> 24));
                }
            }
            WB_CSTAMP(1);
            WB_CSTAMP(2);
            WB_CSTAMP(3);
            return;
        }
    }
    // uint8 images: the tile's source patch (rows r_lo..r_hi, columns c_lo..c_hi of the octave) is
    // first copied to LDS with coalesced dword loads; the 4 taps of every pixel are then LDS byte
    // reads.  (Fetched straight from HBM they were 4 byte-gathers per pixel and the texture-address
    // unit, not the ALUs, set the pace.)  Falls back to direct loads if the patch would not fit
    // (strongly down-scaled tiny levels) and for float32 images.
    bool staged = false;
    int r_lo = 0, c_lo = 0;
    Tap tcs[NCS], trl, tleft;
    trl.i0 = trl.i1 = 0; trl.w0 = trl.w1 = 0.0;
    tleft = trl;
#pragma unroll
    for (int c = 0; c < NCS; ++c) tcs[c] = trl;
    if constexpr (sizeof(T) == 1) {
        // the patch extents: from the host's per-tile table when there is one (wb_channels_launch_x: a scalar load right
        // behind the tile record), else computed here -- four chains of fp64 arithmetic in front of every patch load
        int nrow, nbyte;
        if (a.patches) {
            const WbTilePatch tp = a.patches[blockIdx.x];
            r_lo = tp.r_lo;
            c_lo = tp.c_lo;
            nrow = tp.rows;
            nbyte = tp.bytes;
            staged = nrow != 0;
        } else {
            // (fp64 has no scalar unit: the values are computed by the vector ALU in every lane alike -- said explicitly,
            // so that everything derived from them, the staging loop's buffer descriptor included, stays in scalar registers)
            staged = tile_patch_extent<G, REFLECT>(L, ry0, rx0, rh, r_lo, c_lo, nrow, nbyte);
            r_lo = __builtin_amdgcn_readfirstlane(r_lo);
            c_lo = __builtin_amdgcn_readfirstlane(c_lo);
            nrow = __builtin_amdgcn_readfirstlane(nrow);
            nbyte = __builtin_amdgcn_readfirstlane(nbyte);
        }
        WB_CSTAMP(1);
        // the taps the resample below wants -- a lane's column taps, the row taps of the wave's strip (lane l: its row l), the taps of the
        // RW % 64 right-most columns -- are requested HERE, in front of the patch loads: behind the staging barrier each
        // of these loads was one more exposed memory round trip per workgroup
#pragma unroll
        for (int c = 0; c < NCS; ++c) {
            const int x = tile_coord<REFLECT>(rx0 + lane + 64 * c, L.nw);
            tcs[c] = ctap[x];
        }
        {
            static_assert(wb_strip_rows(RH, NW) <= 64, "one lane per row of the strip");
            const int RS = wb_strip_rows(rh, NW);               // rows of a wave's strip (see the row loop)
            const int kl = wave * RS + lane;
            const int ly = tile_coord<REFLECT>(ry0 + (kl < rh ? kl : rh - 1), L.nh);
            trl = rtap[ly];
            const int lx = tile_coord<REFLECT>(rx0 + MAINW + (lane < LEFT ? lane : 0), L.nw);
            tleft = ctap[lx];
        }
        if (staged) {
            // LDS row r = source row r_lo + r from column c_lo on: dword loads at byte granularity
            // (global memory takes unaligned dwords), aligned LDS stores
            // One patch row per wave at a time, one dword per lane (no index arithmetic per element);
            // UR rows are in flight together.  Lanes past the row end reload its last dword.
            constexpr int DWP = PPITCH / 4;                       // dwords per patch row
            const int ndw = (nbyte + 1 + 3) / 4;                  // + the (i0 + 1) neighbour of the last column
            uint32_t *pw = reinterpret_cast<uint32_t *>(uni);
            constexpr int UR = kChanUR;
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
            for (int dw0 = 0; dw0 < ndw; dw0 += 64) {
                int dw = dw0 + ln;
                dw = dw < ndw ? dw : ndw - 1;
                // a row's address = the patch origin (a buffer descriptor built from wave-uniform values: scalar registers)
                // + the row's byte offset (a scalar: the instruction's soffset) + the lane's byte offset (a 32-bit vector
                // register): the buffer load's own addressing mode -- no 64-bit vector multiply-add per row (round 4; plain
                // pointer arithmetic is folded back into per-lane 64-bit pointers by the compiler)
                const int voff = 4 * dw;
                // (the origin is wave-uniform but the compiler cannot prove it and would wrap every load in a waterfall loop:
                // its two halves go through readfirstlane)
                const uint64_t origin = reinterpret_cast<uint64_t>(src + (int64_t)r_lo * L.src_w + c_lo);
                const uint64_t origin_u = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(origin >> 32)) << 32) |
                                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)origin);
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(origin_u), 0, 0x7fffffff, 0x00020000);
                for (int r0 = wv; r0 < nrow; r0 += NW * UR) {
                    uint32_t v[UR];
                    int rr[UR];
#pragma unroll
                    for (int k = 0; k < UR; ++k) {
                        rr[k] = r0 + NW * k < nrow ? r0 + NW * k : nrow - 1;
                        v[k] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, rr[k] * L.src_w, 0);
                    }
#pragma unroll
                    for (int k = 0; k < UR; ++k) pw[rr[k] * DWP + dw] = v[k];   // duplicates rewrite the same value
                }
            }
            // the row taps of the tile, one entry per tile row: {patch byte offset of the upper tap row, fp32 weights}.
            // Read back below with one wave-uniform (broadcast) LDS load per row: the values arrive in VECTOR registers
            // -- on gfx950 an fp32 add / multiply / fmac whose operands are all vector registers issues in 2 cycles,
            // with a scalar-register operand in 4 (tools/valu_class_probe.hip), and a v_readlane costs 4 as well
            {
                const int RS = wb_strip_rows(rh, NW);
                const int kl = wave * RS + lane;
                if (lane < RS && kl < rh) rowtab[kl] = make_float4(__int_as_float((trl.i0 - r_lo) * PPITCH), (float)trl.w0, (float)trl.w1, 0.0f);
            }
            if (LEFT > 0 && tid >= 64 && tid < 64 + LEFT)
                rowtab[RH + tid - 64] = make_float4(__int_as_float(tleft.i0 - c_lo), (float)tleft.w0, (float)tleft.w1, 0.0f);
            __syncthreads();
        }
    }
    WB_CSTAMP(2);
    if (staged) {
        if constexpr (sizeof(T) == 1) {
            const unsigned char *patch = uni;
            int ci0[NCS];
            float wc0f[NCS], wc1f[NCS];
            const Tap (&tc)[NCS] = tcs;
#pragma unroll
            for (int c = 0; c < NCS; ++c) {
                ci0[c] = tc[c].i0 - c_lo;
                wc0f[c] = (float)tc[c].w0;
                wc1f[c] = (float)tc[c].w1;
            }
            // Each wave owns a strip of consecutive tile rows and walks it RB rows per pass: every tap byte of the pass is
            // requested before the first is used, and the exact redo (fp64, the lane-held fp64 taps -- lane l holds the row
            // taps of row l of the strip: trl) is deferred behind all the fast-path arithmetic, one branch per pass.
            // Consecutive output rows of a down-scale by less than 2 usually share a source row (the lower taps of row k are
            // the upper taps of row k + 1): its horizontal interpolation is then taken over instead of read and computed
            // again; which rows share is wave-uniform.
            // Round 4: the passes are unrolled completely (a strip holds at most RSMAX rows), so nothing is carried
            // around a loop back-edge -- the rolled loop spent 30 of its 88 vector instructions per pass on register moves
            // (next pass's row entries, the previous row's interpolation and tap bytes) --, a pixel's four tap bytes hang
            // off ONE address register (volatile loads, see lds_byte_vol), the tap bytes are not kept for the redo (it reads
            // them again: a redo is rare per pixel), and nothing is left for the SLP vectoriser to pair.
            constexpr int RB = kChanRB;
            constexpr int RSMAX = wb_strip_rows(RH, NW), NPASS = RSMAX / RB;
            const int RS = wb_strip_rows(rh, NW);
            const int k_lo = wave * RS, k_hi = k_lo + RS < rh ? k_lo + RS : rh;
            float hprev[NCS];                     // horizontal interpolation of the patch row at byte offset o_prev
            int o_prev = -1;
#pragma unroll
            for (int c = 0; c < NCS; ++c) hprev[c] = 0.0f;
            auto hlerp = [&](uint8_t x0, uint8_t x1, int c) {
                return scalar_only(__builtin_fmaf((float)x1, wc1f[c], scalar_only((float)x0 * wc0f[c])));
            };
            const int rrow = k_lo * RP + lane;    // this lane's first output of the strip
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) {
                const int k0 = k_lo + RB * ps;
                if (k0 >= k_hi) break;                                          // wave-uniform
                float4 ent[RB];
                int o0[RB], av[RB][NCS];
                bool shared[RB];
                uint8_t b[RB][NCS][4];
                // every load of the pass first, unconditionally (a row past the strip's end repeats the last one; the upper
                // tap pair is fetched even where the previous row's interpolation will stand in for it -- a branch around
                // two byte loads made the compiler wait for them inside the branch, one LDS latency per row)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    int k = k0 + rb;
                    k = k < k_hi ? k : k_hi - 1;
                    ent[rb] = rowtab[k];                                        // wave-uniform address: a broadcast read
                }
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    o0[rb] = __builtin_amdgcn_readfirstlane(__float_as_int(ent[rb].x));
                    // (a00, a01) / (a10, a11) sit at i0, i0 + 1 of two consecutive patch rows; the upper pair's interpolation
                    // is not computed again when it is the previous row's lower pair
                    const int o_above = rb == 0 ? o_prev : o0[rb - 1] + PPITCH;
                    shared[rb] = o0[rb] == o_above;
#pragma unroll
                    for (int c = 0; c < NCS; ++c) {
                        av[rb][c] = ci0[c] + o0[rb];
                        b[rb][c][0] = lds_byte_vol(patch, av[rb][c]);
                        b[rb][c][1] = lds_byte_vol(patch, av[rb][c] + 1);
                        b[rb][c][2] = lds_byte_vol(patch, av[rb][c] + PPITCH);
                        b[rb][c][3] = lds_byte_vol(patch, av[rb][c] + PPITCH + 1);
                    }
                }
                float out[RB][NCS];
                bool need[RB][NCS];
                bool redo = false;
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    float top[NCS];
                    if (shared[rb]) {                                           // wave-uniform
#pragma unroll
                        for (int c = 0; c < NCS; ++c) top[c] = hprev[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < NCS; ++c) top[c] = hlerp(b[rb][c][0], b[rb][c][1], c);
                    }
#pragma unroll
                    for (int c = 0; c < NCS; ++c) {
                        const float bot = hlerp(b[rb][c][2], b[rb][c][3], c);
                        hprev[c] = bot;
                        need[rb][c] = !Src<T>::fast_rows(top[c], bot, ent[rb].y, ent[rb].z, out[rb][c]);
                        redo |= need[rb][c];
                    }
                    o_prev = o0[rb] + PPITCH;
                }
                if (__builtin_amdgcn_ballot_w64(redo) != 0) {              // rare: exact fp64 with the full taps
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        int k = k0 + rb;
                        k = k < k_hi ? k : k_hi - 1;
                        // the row's fp64 weights come from the lane that holds them (no memory access: a load
                        // from the tap table here stalled the whole pass behind an L2 round trip)
                        Tap tr;
                        tr.i0 = tr.i1 = 0;
                        tr.w0 = lane_f64(trl.w0, k - k_lo);
                        tr.w1 = lane_f64(trl.w1, k - k_lo);
#pragma unroll
                        for (int c = 0; c < NCS; ++c) {
                            if (need[rb][c])
                                out[rb][c] = Src<T>::finish(resample_f64((double)b[rb][c][0], (double)b[rb][c][1], (double)b[rb][c][2],
                                                                         (double)b[rb][c][3], tr, tc[c]), mn, mx, a.src_int);
                        }
                    }
                }
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    if (k0 + rb < k_hi) {
#pragma unroll
                        for (int c = 0; c < NCS; ++c) rput(rrow + (RB * ps + rb) * RP + 64 * c, out[rb][c]);
                    }
                }
            }
            // the RW % 64 right-most columns of the wave's own strip, one pixel per lane: row and column entries from the
            // LDS tables, the four tap bytes off one address; coordinates and the fp64 taps only in the (rare) exact redo
            if constexpr (LEFT > 0) {
                const int nleft = (k_hi - k_lo) * LEFT;
                for (int p = lane; p < nleft; p += 64) {
                    const int kk = p / LEFT, q = p - kk * LEFT, k = k_lo + kk;
                    const float4 er = rowtab[k], ec = rowtab[RH + q];
                    const int o = __float_as_int(er.x) + __float_as_int(ec.x);
                    const uint8_t a00 = lds_byte_vol(patch, o), a01 = lds_byte_vol(patch, o + 1);
                    const uint8_t a10 = lds_byte_vol(patch, o + PPITCH), a11 = lds_byte_vol(patch, o + PPITCH + 1);
                    float out = 0.0f;
                    if (!Src<T>::fast((float)a00, (float)a01, (float)a10, (float)a11, er.y, er.z, ec.y, ec.z, out)) {
                        const int y = tile_coord<REFLECT>(ry0 + k, L.nh), x = tile_coord<REFLECT>(rx0 + MAINW + q, L.nw);
                        const Tap tr = rtap[y], tcl = ctap[x];
                        out = Src<T>::finish(resample_f64((double)a00, (double)a01, (double)a10, (double)a11, tr, tcl), mn, mx, a.src_int);
                    }
                    rput(k * RP + MAINW + q, out);
                }
            }
        }
    } else
    {
        Tap tc[NCS];
        float wc0f[NCS], wc1f[NCS];
#pragma unroll
        for (int c = 0; c < NCS; ++c) {
            const int x = tile_coord<REFLECT>(rx0 + lane + 64 * c, L.nw);
            tc[c] = ctap[x];
            wc0f[c] = (float)tc[c].w0;
            wc1f[c] = (float)tc[c].w1;
        }
        // RB rows per pass: all their source loads are in flight before the first one is used
        // (one row at a time, the loop was a chain of RH/4 memory latencies per wave)
        constexpr int RB = sizeof(T) == 8 ? 2 : 5;             // (a double pixel is two registers)
        for (int k0 = wave; k0 < rh; k0 += NW * RB) {
            Tap tr[RB];
            T v00[RB][NCS], v01[RB][NCS], v10[RB][NCS], v11[RB][NCS];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                int k = k0 + NW * rb;
                k = k < rh ? k : rh - 1;                                  // clamped, unconditional loads
                const int y = tile_coord<REFLECT>(ry0 + k, L.nh);
                tr[rb] = rtap[__builtin_amdgcn_readfirstlane(y)];
                const T *r0 = src + (int64_t)__builtin_amdgcn_readfirstlane(tr[rb].i0) * L.src_w;
                const T *r1 = src + (int64_t)__builtin_amdgcn_readfirstlane(tr[rb].i1) * L.src_w;
#pragma unroll
                for (int c = 0; c < NCS; ++c) {
                    v00[rb][c] = r0[tc[c].i0];
                    v01[rb][c] = r0[tc[c].i1];
                    v10[rb][c] = r1[tc[c].i0];
                    v11[rb][c] = r1[tc[c].i1];
                }
            }
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int k = k0 + NW * rb;
#pragma unroll
                for (int c = 0; c < NCS; ++c) {
                    float out = 0.0f;
                    if (ident && Src<T>::taps_finite(v01[rb][c], v10[rb][c], v11[rb][c])) {
                        // (float32 / integer results pass the clip unchanged: the pixel lies in its octave's range;
                        // a NaN bound turns every pixel of the level into NaN, also the copied ones)
                        out = (mn != mn || mx != mx) ? __builtin_nanf("") : (float)v00[rb][c];
                    } else {
                        bool ok = false;
                        if constexpr (Src<T>::kFastResample)
                            ok = Src<T>::fast((float)v00[rb][c], (float)v01[rb][c], (float)v10[rb][c], (float)v11[rb][c],
                                              (float)tr[rb].w0, (float)tr[rb].w1, wc0f[c], wc1f[c], out);
                        if (!ok)
                            out = Src<T>::finish(resample_f64((double)v00[rb][c], (double)v01[rb][c], (double)v10[rb][c],
                                                              (double)v11[rb][c], tr[rb], tc[c]), mn, mx, a.src_int);
                    }
                    if (k < rh) rput(k * RP + lane + 64 * c, out);
                }
            }
        }
    }
    WB_CSTAMP(3);
    if constexpr (LEFT > 0) {
        // (a staged tile has done these columns wave by wave above)
        for (int p = staged ? rh * LEFT : tid; p < rh * LEFT; p += NT) {
            const int k = p / LEFT, q = MAINW + p - k * LEFT;
            const int y = tile_coord<REFLECT>(ry0 + k, L.nh), x = tile_coord<REFLECT>(rx0 + q, L.nw);
            float out = 0.0f;
            bool ok = false;
            const Tap tr = rtap[y], tc = ctap[x];
            const T *r0 = src + (int64_t)tr.i0 * L.src_w;
            const T *r1 = src + (int64_t)tr.i1 * L.src_w;
            const T a00 = r0[tc.i0], a01 = r0[tc.i1], a10 = r1[tc.i0], a11 = r1[tc.i1];
            ok = ident && Src<T>::taps_finite(a01, a10, a11);
            if (ok) out = (mn != mn || mx != mx) ? __builtin_nanf("") : (float)a00;
            if constexpr (Src<T>::kFastResample)
                if (!ok) ok = Src<T>::fast((float)a00, (float)a01, (float)a10, (float)a11, (float)tr.w0, (float)tr.w1,
                                           (float)tc.w0, (float)tc.w1, out);
            if (!ok) out = Src<T>::finish(resample_f64((double)a00, (double)a01, (double)a10, (double)a11, tr, tc), mn, mx, a.src_int);
            rput(k * RP + q, out);
        }
    }
}

// ---- the output tile (and the threads) of every channel kernel, in this one place: template arguments and the host's
//      patch table take it at compile time, wb_channels_tile answers from it at run time.  16 x 64 at shrink 1 and 2; 8 x 32
//      at shrink 4 -- but 8 x 30 for grad_hist: the shrunk tile with its smooth halo is then 10 x 32 = 320 pixels = five full
//      waves of step 2 (8 x 32: 340, a sixth wave for twenty lanes), the resized tile 130 columns = two per lane + 2 (138: + 10)
struct ChanTile {
    int tu, tv, nt;
};
constexpr ChanTile chan_tile(int channel_func, int shrink) {
    return {shrink == 4 ? 8 : 16, shrink != 4 ? 64 : channel_func == WB_CHN_GRAD_HIST ? 30 : 32, channel_func == WB_CHN_GRAD_MAG ? 512 : 256};
}

// ---- run-time (shrink, smooth) -> compile-time constants: f(std::integral_constant<int, S>{}, std::bool_constant<SMOOTH>{}),
//      whose int result is handed back; `who` names the entry point in the one error for a shrink without kernels
template <typename F> int chan_dispatch(const char *who, int shrink, bool smooth, F &&f) {
    auto with_smooth = [&](auto s) { return smooth ? f(s, std::true_type{}) : f(s, std::false_type{}); };
    switch (shrink) {
        case 1: return with_smooth(std::integral_constant<int, 1>{});
        case 2: return with_smooth(std::integral_constant<int, 2>{});
        case 4: return with_smooth(std::integral_constant<int, 4>{});
    }
    wb_set_error("%s: shrink=%d unsupported (1, 2; 4 as an extension)", who, shrink);
    return WB_ERR_UNSUPPORTED;
}

}  // namespace
