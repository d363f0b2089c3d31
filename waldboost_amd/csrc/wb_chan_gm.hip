// waldboost.channels.grad_mag (reference channels.py:11-37, defaults norm=5, eps=1e-3): one float32
// channel  mag / (triangle11(mag) + eps),  mag = sqrt(gx^2 + gy^2) in fp32.  The normaliser is
// scipy's convolve1d twice (rows, then columns) with the 11-tap triangle: symmetric-kernel branch
// of NI_Correlate1D, fp64 accumulation  t = x[l]*w[c];  t += (x[l+j] + x[l-j]) * w[c+j], j = -5..-1,
// one fp32 rounding per pass, 'reflect' borders.  The tile therefore carries a 5-pixel halo of mag
// (6 of the resized image); halo positions outside the level hold the REFLECTED coordinate's
// pixel, under which the gradient magnitude of the mirror position comes out exactly (the [1,2,1]
// pass is symmetric, the difference pass only changes sign).  Secondary channel function: plain
// per-pixel code, not tuned like channels_kernel.
// (channels_gm_kernel and its launcher; step 1 is the shared resample_tile of wb_chan_tile.h with mirrored coordinates)
#include "wb_chan_tile.h"

namespace {

struct GmGeom {
    static constexpr int NH = 5;      // half width of the 11-tap triangle
};

// (the geometry resample_tile wants: the resized tile and the staged source patch -- uint8 images, any down-scale
// below 2 -- which shares its memory with the magnitudes and the shrunk tile, both written after the resize)
template <int S, int TU, int TV, bool SMOOTH> struct GmTile {
    static constexpr int HS = SMOOTH ? 1 : 0, NH = GmGeom::NH;
    static constexpr int SU = TU + 2 * HS, SV = TV + 2 * HS;      // shrunk tile incl. smooth halo
    static constexpr int VH = S * SU, VW = S * SV;                // normalised magnitudes needed
    static constexpr int MH = VH + 2 * NH, MW = VW + 2 * NH;      // magnitudes incl. the triangle halo
    static constexpr int RH = MH + 2, RW = MW + 2;                // resized pixels incl. the gradient halo
    // (512 threads: at two workgroups per CU -- what the 60 KB of LDS admit -- 16 waves per CU, like the gradient kernels)
    static constexpr int NT = 512, NW = NT / 64;
    static constexpr int PROWS = 2 * RH + 4, PPITCH = (2 * RW + 12 + 3) & ~3;
};

template <typename T, int S, int TU, int TV, bool SMOOTH>
__global__ __launch_bounds__(512, 2) void channels_gm_kernel(ChanArgs a) {
    using G = GmTile<S, TU, TV, SMOOTH>;
    constexpr int HS = G::HS, NH = G::NH, SU = G::SU, SV = G::SV, VH = G::VH, VW = G::VW, MH = G::MH, MW = G::MW;
    constexpr int RH = G::RH, RW = G::RW, NT = G::NT;
    constexpr int MG_SH_BYTES = (MH * MW + SU * SV) * 4, PATCH_BYTES = sizeof(T) == 1 ? G::PROWS * G::PPITCH : 0;
    __shared__ __attribute__((aligned(16))) float R[RH * RW];   // resized tile; later the row-pass result [VH][MW]
    __shared__ __attribute__((aligned(16))) unsigned char uni[MG_SH_BYTES > PATCH_BYTES ? MG_SH_BYTES : PATCH_BYTES];
    __shared__ float4 rowtab[sizeof(T) == 1 ? RH + RW % 64 : 1];
    float *Mg = reinterpret_cast<float *>(uni);            // magnitudes; the centre is normalised in place
    float *Sh = Mg + MH * MW;
    static_assert(VH * MW <= RH * RW, "row-pass result reuses the resized tile");

    const WbTile tile = a.tiles[blockIdx.x];
    const WbLevel L = a.levels[tile.level];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int u0 = tile.ty * TU, v0 = tile.tx * TV;
    const T *src = (L.oct == 0) ? (const T *)a.img + (int64_t)b * a.img_stride
                                : (const T *)a.oct + (int64_t)b * a.oct_stride + L.src_off;
    double mn, mx;
    clip_range<T>(a, b, L.oct, mn, mx);
    const int ry0 = S * (u0 - HS) - NH - 1, rx0 = S * (v0 - HS) - NH - 1;

    // ---- resized pixels (reference channels.py:132), reflected outside the level: the channel kernels' own resample
    //      (uint8: source patch staged in LDS, shared interpolation between rows, exact redo where the fast path's
    //      band test asks for it) with mirrored instead of clamped coordinates
    resample_tile<T, G, true>(a, L, src, mn, mx, ry0, rx0, RH, R, uni, rowtab, tid);
    __syncthreads();
    if (a.dbg & 1) return;           // (WB_CHAN_DBG: phase timing -- 1 resize, 2 magnitudes, 8 / 16 the two triangle passes)

    // ---- gradient magnitude (channels.py:16-21, 31-32): fp32 squares, sum and square root
    for (int p = tid; p < MH * MW; p += NT) {
        const int k = p / MW, q = p - k * MW;
        const float *c = R + k * RW + q;                      // 3x3 patch, centre at (k+1, q+1)
        const float hc0 = Src<T>::hpass(c[0], c[RW], c[2 * RW]);              // vertical [1,2,1] at column q
        const float hc2 = Src<T>::hpass(c[2], c[RW + 2], c[2 * RW + 2]);      //                     column q+2
        const float hr0 = Src<T>::hpass(c[0], c[1], c[2]);                    // horizontal [1,2,1] at row k
        const float hr2 = Src<T>::hpass(c[2 * RW], c[2 * RW + 1], c[2 * RW + 2]);
        const float hc1 = Src<T>::hpass(c[1], c[RW + 1], c[2 * RW + 1]);      // the centre taps (weight 0: see dpass)
        const float hr1 = Src<T>::hpass(c[RW], c[RW + 1], c[RW + 2]);
        const float gx = Src<T>::dpass(hc0, hc1, hc2), gy = Src<T>::dpass(hr0, hr1, hr2);
        Mg[p] = sqrtf(gx * gx + gy * gy);
    }
    __syncthreads();
    if (a.dbg & 2) return;

    // ---- triangle filter along the rows' axis (convolve1d axis 0), result over the resized tile's memory.
    //      Each thread forms TG outputs that are neighbours ALONG the filter: the 10 + TG magnitudes they span are read
    //      and widened to fp64 once (one output at a time, every magnitude was read and converted eleven times);
    //      per output the sum is formed exactly as before, term by term in scipy's order.
    constexpr int TG = 4;
    float *Tv = R;
    {
        constexpr int GROUPS = (VH + TG - 1) / TG;
        for (int p = tid; p < GROUPS * MW; p += NT) {
            const int g = p / MW, q = p - g * MW, k0 = g * TG;
            double x[TG + 2 * NH];
#pragma unroll
            for (int i = 0; i < TG + 2 * NH; ++i) {
                const int row = k0 + i < MH ? k0 + i : MH - 1;     // (rows past the tile: read, never used)
                x[i] = (double)Mg[row * MW + q];
            }
#pragma unroll
            for (int o = 0; o < TG; ++o) {
                if (k0 + o >= VH) break;
                double t = x[o + NH] * a.tri[NH];
#pragma unroll
                for (int j = -NH; j < 0; ++j) t = t + (x[o + NH + j] + x[o + NH - j]) * a.tri[NH + j];
                Tv[(k0 + o) * MW + q] = (float)t;
            }
        }
    }
    __syncthreads();
    if (a.dbg & 8) return;
    // ---- ... along the columns' axis, then mag / (norm + eps), in place at the centre of Mg
    {
        constexpr int GROUPS = (VW + TG - 1) / TG;
        for (int p = tid; p < VH * GROUPS; p += NT) {
            // (neighbouring lanes take neighbouring ROWS: their reads are MW floats apart -- 2-way bank conflicts; TG
            // floats apart, along the row, they were 4-way)
            const int qg = p / VH, k = p - qg * VH, q0 = qg * TG;
            double x[TG + 2 * NH];
#pragma unroll
            for (int i = 0; i < TG + 2 * NH; ++i) {
                const int col = q0 + i < MW ? q0 + i : MW - 1;
                x[i] = (double)Tv[k * MW + col];
            }
#pragma unroll
            for (int o = 0; o < TG; ++o) {
                if (q0 + o >= VW) break;
                double t = x[o + NH] * a.tri[NH];
#pragma unroll
                for (int j = -NH; j < 0; ++j) t = t + (x[o + NH + j] + x[o + NH - j]) * a.tri[NH + j];
                float *m = Mg + (k + NH) * MW + q0 + o + NH;
                *m = *m / ((float)t + a.gm_eps);
            }
        }
    }
    __syncthreads();
    if (a.dbg & 16) return;

    // ---- shrink (channels.py:55-64, fp32 ((a+b)+c)+d then /4)
    for (int p = tid; p < SU * SV; p += NT) {
        const int i = p / SV, j = p - i * SV;
        auto at = [&](int y, int x) { return Mg[(S * i + y + NH) * MW + S * j + x + NH]; };
        float o;
        if constexpr (S == 1) {
            o = at(0, 0);
        } else if constexpr (S == 2) {
            o = (((at(0, 0) + at(1, 0)) + at(0, 1)) + at(1, 1)) * 0.25f;
        } else {
            float qd[2][2];
#pragma unroll
            for (int A = 0; A < 2; ++A)
#pragma unroll
                for (int B = 0; B < 2; ++B)
                    qd[A][B] = (((at(2 * A, 2 * B) + at(2 * A + 1, 2 * B)) + at(2 * A, 2 * B + 1)) + at(2 * A + 1, 2 * B + 1)) * 0.25f;
            o = (((qd[0][0] + qd[1][0]) + qd[0][1]) + qd[1][1]) * 0.25f;
        }
        Sh[p] = o;
    }
    __syncthreads();

    // ---- 3x3 smooth (fp64, source order), border 0, store [u][v][1]
    float *out = reinterpret_cast<float *>(a.chn) + (int64_t)b * a.chn_stride + L.chn_off;
    for (int p = tid; p < TU * TV; p += NT) {
        const int i = p / TV, j = p - i * TV;
        const int su = u0 + i, sv = v0 + j;
        if (su >= L.u || sv >= L.v) continue;
        float o;
        if constexpr (SMOOTH) {
            const float *c = Sh + i * SV + j;
            o = smooth9(c[0], c[1], c[2], c[SV], c[SV + 1], c[SV + 2], c[2 * SV], c[2 * SV + 1], c[2 * SV + 2]);
            if (su == 0 || sv == 0 || su == L.u - 1 || sv == L.v - 1) o = 0.0f;
        } else {
            o = Sh[i * SV + j];
        }
        out[(int64_t)su * L.v + sv] = o;
    }
}


template <typename T>
int launch_gm(hipStream_t st, dim3 grid, const ChanArgs &a, int shrink, bool smooth) {
    return chan_dispatch("wb_channels_launch", shrink, smooth, [&](auto s, auto sm) {
        constexpr int S = decltype(s)::value;
        constexpr ChanTile t = chan_tile(WB_CHN_GRAD_MAG, S);
        static_assert(t.nt == GmTile<S, t.tu, t.tv, true>::NT, "workgroup size");
        hipLaunchKernelGGL((channels_gm_kernel<T, S, t.tu, t.tv, decltype(sm)::value>), grid, dim3(t.nt), 0, st, a);
        WB_HIP_CHECK(hipGetLastError());
        return WB_OK;
    });
}

}  // namespace

int wb_chan_launch_gm(hipStream_t st, dim3 grid, const void *chan_args, int dtype, int shrink, bool smooth) {
    const ChanArgs &a = *static_cast<const ChanArgs *>(chan_args);
    if (dtype == WB_DTYPE_U8) return launch_gm<uint8_t>(st, grid, a, shrink, smooth);
    if (dtype == WB_DTYPE_F32) return launch_gm<float>(st, grid, a, shrink, smooth);
    wb_set_error("wb_channels_launch: unsupported dtype %d (uint8 and float32 images only)", dtype);
    return WB_ERR_UNSUPPORTED;
}
