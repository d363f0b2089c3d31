// Integer channel functions of the reference's FPGA flavour (fpga/channels.py:5-67) on uint8 images:
//   dx, dy   3x3 Sobel stencils in exact integer arithmetic; numba leaves the 1-pixel border of
//            the (resized) image at 0 -- no reflected halo here
//   NCH = 4  grad_hist_4_u1: y = (dx, trunc((dx-dy)/2), dy, trunc((dx+dy)/2)); min(|y| // 4, 255)
//   NCH = 1  grad_mag_u1:    min(max(|dx|, |dy|) // 4, 255)
// then channel_pyramid's generic tail on uint8 arrays: avg_pool_2 wraps its three uint8 adds
// mod 256 before the /4 (channels.py:61-64), the smooth stencil sums in int64 and the /16 is
// truncated by the store into the uint8 array (channels.py:78-90), border 0.
// Output [u][v][NCH] uint8: one dword (NCH = 4) or one byte per pixel.
// (channels_u1_kernel and its launcher; step 1 and the tile geometry are the shared ones of wb_chan_tile.h)
#include "wb_chan_tile.h"

namespace {

template <int S, int TU, int TV, bool SMOOTH, int NCH>
__global__ __launch_bounds__(256) void channels_u1_kernel(ChanArgs a) {
    using T = uint8_t;
    using G = TileGeom<S, TU, TV, SMOOTH>;
    constexpr int HS = G::HS, SU = G::SU, SV = G::SV, RH = G::RH, RW = G::RW, P = G::P;
    constexpr int UNI_BYTES = G::SH_BYTES > G::PATCH_BYTES ? G::SH_BYTES : G::PATCH_BYTES;
    __shared__ float R[RH * RW];
    __shared__ __attribute__((aligned(16))) unsigned char uni[UNI_BYTES];
    __shared__ float4 rowtab[RH + RW % 64];
    uint32_t *Sh = reinterpret_cast<uint32_t *>(uni);     // packed channels of one shrunk pixel

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
    resample_tile<T, G>(a, L, src, mn, mx, ry0, rx0, RH, R, uni, rowtab, tid);
    __syncthreads();
    if (a.dbg & 1) return;

    // ---- step 2: integer gradients -> channels -> shrink, one shrunk pixel per iteration
    for (int p = tid; p < SU * SV; p += 256) {
        const int i = p / SV, j = p - i * SV;
        // The stencils in fp32 (exact: integers below 2^11), shared [1,2,1] passes as in channels_kernel;
        // only the channel values are converted to integers.  trunc((dx -/+ dy) / 2) has the magnitude
        // floor(|dx -/+ dy| / 2), so  |y| // 4  is  |dx| >> 2, |dx - dy| >> 3, |dy| >> 2, |dx + dy| >> 3;
        // with 8 bit pixels |dx|, |dy| <= 1020, so none of them exceeds 255 and the clamp never acts.
        float pt[P][P];
#pragma unroll
        for (int y = 0; y < P; ++y)
#pragma unroll
            for (int x = 0; x < P; ++x) pt[y][x] = R[(S * i + y) * RW + (S * j + x)];
        float hc[S][P], hr[P][S];
#pragma unroll
        for (int y = 0; y < S; ++y)
#pragma unroll
            for (int x = 0; x < P; ++x) hc[y][x] = scalar_only(Src<T>::hpass(pt[y][x], pt[y + 1][x], pt[y + 2][x]));
#pragma unroll
        for (int y = 0; y < P; ++y)
#pragma unroll
            for (int x = 0; x < S; ++x) hr[y][x] = scalar_only(Src<T>::hpass(pt[y][x], pt[y][x + 1], pt[y][x + 2]));
        // numba leaves the 1-pixel border of the resized image at 0: only blocks on that border test their pixels
        const int by0 = ry0 + S * i + 1, bx0 = rx0 + S * j + 1;                    // first pixel of the block
        const bool on_border = by0 <= 0 || bx0 <= 0 || by0 + S - 1 >= L.nh - 1 || bx0 + S - 1 >= L.nw - 1;
        int ch[S][S][NCH];
#pragma unroll
        for (int y = 0; y < S; ++y)
#pragma unroll
            for (int x = 0; x < S; ++x) {
                float dx = scalar_only(hc[y][x + 2] - hc[y][x]);
                float dy = scalar_only(hr[y + 2][x] - hr[y][x]);
                if (on_border) {
                    const int gy = by0 + y, gx = bx0 + x;
                    if (gy <= 0 || gx <= 0 || gy >= L.nh - 1 || gx >= L.nw - 1) dx = dy = 0.0f;
                }
                if constexpr (NCH == 4) {
                    ch[y][x][0] = (int)(uint32_t)fabsf(dx) >> 2;
                    ch[y][x][1] = (int)(uint32_t)fabsf(dx - dy) >> 3;
                    ch[y][x][2] = (int)(uint32_t)fabsf(dy) >> 2;
                    ch[y][x][3] = (int)(uint32_t)fabsf(dx + dy) >> 3;
                } else {
                    ch[y][x][0] = (int)(uint32_t)fmaxf(fabsf(dx), fabsf(dy)) >> 2;
                }
            }
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            int v;
            if constexpr (S == 1) {
                v = ch[0][0][k];
            } else if constexpr (S == 2) {
                v = ((ch[0][0][k] + ch[1][0][k] + ch[0][1][k] + ch[1][1][k]) & 255) >> 2;
            } else {  // S == 4 (extension): avg_pool_2 applied twice
                int q[2][2];
#pragma unroll
                for (int A = 0; A < 2; ++A)
#pragma unroll
                    for (int B = 0; B < 2; ++B)
                        q[A][B] = ((ch[2 * A][2 * B][k] + ch[2 * A + 1][2 * B][k] + ch[2 * A][2 * B + 1][k] +
                                    ch[2 * A + 1][2 * B + 1][k]) & 255) >> 2;
                v = ((q[0][0] + q[1][0] + q[0][1] + q[1][1]) & 255) >> 2;
            }
            o |= (uint32_t)v << (8 * k);
        }
        Sh[p] = o;
    }
    __syncthreads();
    if (a.dbg & 2) return;

    // ---- step 3: 3x3 binomial smooth, integer sum >> 4, border = 0; strips as in channels_kernel
    constexpr int RPT = TU * TV / 256;
    static_assert(TU * TV % 256 == 0 && 256 % TV == 0, "tile must split into whole thread strips");
    uint8_t *out = reinterpret_cast<uint8_t *>(a.chn) + (int64_t)b * a.chn_stride + L.chn_off;
    const int j = tid % TV, i0 = (tid / TV) * RPT;
    const int sv = v0 + j;
    uint32_t o[RPT];
    if constexpr (SMOOTH) {
        uint32_t w[RPT + 2][3];
#pragma unroll
        for (int y = 0; y < RPT + 2; ++y)
#pragma unroll
            for (int x = 0; x < 3; ++x) w[y][x] = Sh[(i0 + y) * SV + (j + x)];
#pragma unroll
        for (int y = 0; y < RPT; ++y) {
            o[y] = 0;
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                auto at = [&](int yy, int xx) { return (int)((w[y + yy][xx] >> (8 * k)) & 255u); };
                const int sum = at(0, 0) + 2 * at(0, 1) + at(0, 2) + 2 * at(1, 0) + 4 * at(1, 1) + 2 * at(1, 2) +
                                at(2, 0) + 2 * at(2, 1) + at(2, 2);
                o[y] |= (uint32_t)(sum >> 4) << (8 * k);
            }
        }
    } else {
#pragma unroll
        for (int y = 0; y < RPT; ++y) o[y] = Sh[(i0 + y) * SV + j];
    }
#pragma unroll
    for (int y = 0; y < RPT; ++y) {
        const int su = u0 + i0 + y;
        if (su >= L.u || sv >= L.v || (a.dbg & 4)) continue;
        if (SMOOTH && (su == 0 || sv == 0 || su == L.u - 1 || sv == L.v - 1)) o[y] = 0;
        const int64_t at = (int64_t)su * L.v + sv;
        if constexpr (NCH == 4)
            reinterpret_cast<uint32_t *>(out)[at] = o[y];        // 64 lanes store 256 B contiguous
        else
            out[at] = (uint8_t)o[y];
    }
}


template <int FUNC, int NCH>
int launch_u1(hipStream_t st, dim3 grid, const ChanArgs &a, int shrink, bool smooth) {
    return chan_dispatch("wb_channels_launch", shrink, smooth, [&](auto s, auto sm) {
        constexpr int S = decltype(s)::value;
        constexpr ChanTile t = chan_tile(FUNC, S);
        hipLaunchKernelGGL((channels_u1_kernel<S, t.tu, t.tv, decltype(sm)::value, NCH>), grid, dim3(t.nt), 0, st, a);
        WB_HIP_CHECK(hipGetLastError());
        return WB_OK;
    });
}

}  // namespace

int wb_chan_launch_u1(hipStream_t st, dim3 grid, const void *chan_args, int channel_func, int shrink, bool smooth) {
    const ChanArgs &a = *static_cast<const ChanArgs *>(chan_args);
    return channel_func == WB_CHN_GRAD_HIST_4_U1 ? launch_u1<WB_CHN_GRAD_HIST_4_U1, 4>(st, grid, a, shrink, smooth)
                                                 : launch_u1<WB_CHN_GRAD_MAG_U1, 1>(st, grid, a, shrink, smooth);
}
