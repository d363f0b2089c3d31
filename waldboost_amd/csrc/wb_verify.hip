// CNN re-scoring of detection windows (wb_verify_launch): the forward pass of the reference's verification.model_cnn
// (reference verification.py:28-56) on crops [N][m][n][C], result = cnn(crop) + score.
//
// Arithmetic contract (tests/verify_reference.py is its NumPy statement, DESIGN section 4.10 its prose):
//   * conv 3x3 "same" C->8, ReLU; conv 8->8, ReLU; 2x2 max pool (floor); conv 8->16, ReLU; conv 16->16, ReLU; flatten in
//     (row, column, channel) order; dense F->128, ReLU; dense 128->1; + score.  Batch normalisation is folded into the
//     convolutions on the host: the kernels see W' and b' only.
//   * every pre-activation is ONE float32 chain: acc = b', then acc = fmaf(x_k, w_k, acc), k ascending, one rounding per
//     step.  Convolution order: ky, kx, input channel (fastest); dense order: the flat input index.  No split-K, no
//     atomics, one accumulator per output: a window's result does not depend on the batch or on its place in it.
//   * taps outside the window are multiplied by zero (fmaf(0, w, acc) == acc for finite w, up to the sign of a zero that
//     the ReLU removes); ReLU is acc > 0 ? acc : +0; the final + score is one float32 add.
//   This file is built with -ffp-contract=off like the rest: every fused multiply-add is a written __builtin_fmaf or the
//   f32 matrix instruction, which on gfx950 is bit for bit the k-ordered fmaf chain (k = 0 of lanes 0..31 before k = 1 of
//   lanes 32..63; tests/test_gpu_verify*.py hold it to that).
//
// Two kernels.
//   verify_front_kernel: `pack` windows per workgroup of 256.  Activations live in LDS, channel-planar ([channel][pixel]:
//     neighbouring lanes read neighbouring words), in two buffers per window: b0 = max(C, 8) planes of m * n, b1 = 8
//     planes.  crop -> b0, conv1 b0 -> b1, conv2 b1 -> b0, pool b0 -> b1, conv3 b1 -> b0, conv4 b0 -> features [N][F] in
//     global memory.  A thread owns one output pixel and all 8 / 16 output channels of it: one LDS read feeds 8 / 16 fmaf,
//     and the weights of a step are the same address in every lane, so they come through the scalar cache (s_load_dwordx8
//     / x16) and take no LDS and no vector register beyond the accumulators.
//   verify_back_kernel: [N][F] x [F][128] as a tiled GEMM on v_mfma_f32_32x32x2_f32, 64 windows x 128 columns per
//     workgroup: wave w owns columns 32 w .. 32 w + 31 and two 32 x 32 accumulator tiles (windows 0..31 and 32..63),
//     initialised with the bias.  The A operand (features) is staged through LDS 16 k at a time, double buffered, one
//     barrier per stage; the B operand (the dense kernel, L2 resident) is read straight from global memory, 256
//     contiguous bytes per wave and k-step.  Epilogue: ReLU into an LDS tile, then 64 threads run the 128-long chain of
//     the last layer and add the score.
// Rows behind the last window are clamped to it on load and never written, so nothing in the scratch needs clearing.
#include "wb_common.h"

#define WB_VERIFY_MAX_SIDE 32
#define WB_VERIFY_MAX_C 16
#define WB_VERIFY_HIDDEN 128
#define WB_VERIFY_MAX_WINDOWS (1 << 26)
#define WB_VERIFY_PACK_MAX 8                    // most windows of one front workgroup
#define WB_VERIFY_PACK_LDS (64 * 1024)          // LDS several windows may share (one window may take more)
#define WB_VERIFY_FRONT_LDS_MAX (128 * 1024)    // 32 x 32 x 16: 24 planes of 4 KiB = 96 KiB
#define WB_VERIFY_TILE 64                       // windows of one back workgroup
#define WB_VERIFY_KC 16                         // k staged per barrier; F is a multiple of 16
#define WB_VERIFY_APITCH (WB_VERIFY_KC + 1)
#define WB_VERIFY_HPITCH (WB_VERIFY_HIDDEN + 1)

namespace {

// offsets (in floats) of the packed weight buffer: include/waldboost_hip.h documents the layout
struct VerifyLayout {
    int m, n, C, m2, n2, F;
    int64_t conv_w[4], conv_b[4], dense0_w, dense0_b, dense1_w, dense1_b, count;
    int pack;           // windows per front workgroup
    int win_floats;     // LDS floats of one window
};

int verify_layout(int m, int n, int C, VerifyLayout *L, const char *who) {
    if (m < 2 || n < 2 || m > WB_VERIFY_MAX_SIDE || n > WB_VERIFY_MAX_SIDE || C < 1 || C > WB_VERIFY_MAX_C) {
        wb_set_error("%s: window shape (%d, %d, %d): supported are 2 <= m, n <= %d and 1 <= C <= %d", who, m, n, C,
                     WB_VERIFY_MAX_SIDE, WB_VERIFY_MAX_C);
        return WB_ERR_UNSUPPORTED;
    }
    L->m = m, L->n = n, L->C = C, L->m2 = m / 2, L->n2 = n / 2, L->F = L->m2 * L->n2 * 16;
    const int cin[4] = {C, 8, 8, 16}, cout[4] = {8, 8, 16, 16};
    int64_t at = 0;
    for (int k = 0; k < 4; ++k) {
        L->conv_w[k] = at, at += 9 * cin[k] * cout[k];
        L->conv_b[k] = at, at += cout[k];
    }
    L->dense0_w = at, at += (int64_t)L->F * WB_VERIFY_HIDDEN;
    L->dense0_b = at, at += WB_VERIFY_HIDDEN;
    L->dense1_w = at, at += WB_VERIFY_HIDDEN;
    L->dense1_b = at, at += 1;
    L->count = at;
    L->win_floats = m * n * ((C > 8 ? C : 8) + 8);
    int pack = 256 / (L->m2 * L->n2);                                   // the pooled layers fill the workgroup
    const int fit = WB_VERIFY_PACK_LDS / (L->win_floats * 4);
    if (pack > fit) pack = fit;
    if (pack > WB_VERIFY_PACK_MAX) pack = WB_VERIFY_PACK_MAX;
    L->pack = pack < 1 ? 1 : pack;
    return WB_OK;
}

// One 3x3 "same" convolution + ReLU over `nwin` windows of H x W pixels: in [window][CIN planes of H * W] in LDS;
// out either LDS planes (COUT of them) or, TO_GLOBAL, the feature rows [window][pixel][COUT] in global memory.
// w: [ky][kx][cin][COUT], b: [COUT], global memory read at wave-uniform addresses.
template <int COUT, bool TO_GLOBAL>
__device__ inline void verify_conv(const float *in, int in_stride, float *out, size_t out_stride, const float *__restrict__ w,
                                   const float *__restrict__ b, int cin, int H, int W, int nwin) {
    const int P = H * W;
    for (int item = threadIdx.x; item < nwin * P; item += 256) {
        const int wi = item / P, p = item - wi * P;
        const int y = p / W, x = p - y * W;
        const float *src = in + wi * in_stride;
        float acc[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = b[o];
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll 1
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = y + ky - 1, xx = x + kx - 1;
                const bool inside = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                const int at = inside ? yy * W + xx : 0;
                const float *wt = w + (ky * 3 + kx) * cin * COUT;
#pragma unroll 4
                for (int i = 0; i < cin; ++i) {
                    float v = src[i * P + at];            // (always read: the clamped address is inside the window)
                    v = inside ? v : 0.0f;
#pragma unroll
                    for (int o = 0; o < COUT; ++o) acc[o] = __builtin_fmaf(v, wt[i * COUT + o], acc[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = acc[o] > 0.0f ? acc[o] : 0.0f;
        if (TO_GLOBAL) {
            float4 *dst = reinterpret_cast<float4 *>(out + wi * out_stride + (size_t)p * COUT);
#pragma unroll
            for (int o = 0; o < COUT; o += 4) dst[o / 4] = make_float4(acc[o], acc[o + 1], acc[o + 2], acc[o + 3]);
        } else {
            float *dst = out + wi * out_stride + p;
#pragma unroll
            for (int o = 0; o < COUT; ++o) dst[o * P] = acc[o];
        }
    }
}

__global__ __launch_bounds__(256) void verify_front_kernel(const void *X, int x_u8, int N, int m, int n, int C, int pack,
                                                           const float *__restrict__ wts, VerifyLayout L, float *feat) {
    extern __shared__ float lds[];
    const int P = m * n, m2 = m >> 1, n2 = n >> 1, P2 = m2 * n2;
    const int s0 = P * (C > 8 ? C : 8), s1 = P * 8;          // floats per window of the two buffers
    float *b0 = lds, *b1 = lds + pack * s0;
    const int win0 = blockIdx.x * pack;
    const int nwin = N - win0 < pack ? N - win0 : pack;
    // crop [pixel][channel] -> b0 [channel][pixel]; uint8 widens exactly
    const int per = P * C;
    const size_t base = (size_t)win0 * per;
    for (int e = threadIdx.x; e < nwin * per; e += 256) {
        const int wi = e / per, r = e - wi * per;
        const int p = r / C, c = r - p * C;
        const float v = x_u8 ? (float)static_cast<const uint8_t *>(X)[base + e] : static_cast<const float *>(X)[base + e];
        b0[wi * s0 + c * P + p] = v;
    }
    __syncthreads();
    verify_conv<8, false>(b0, s0, b1, s1, wts + L.conv_w[0], wts + L.conv_b[0], C, m, n, nwin);
    __syncthreads();
    verify_conv<8, false>(b1, s1, b0, s0, wts + L.conv_w[1], wts + L.conv_b[1], 8, m, n, nwin);
    __syncthreads();
    // 2x2 max pool, stride 2, the last row / column of an odd size dropped: b0 [8][P] -> b1 [8][P2]
    for (int item = threadIdx.x; item < nwin * 8 * P2; item += 256) {
        const int wi = item / (8 * P2), r = item - wi * 8 * P2;
        const int c = r / P2, p2 = r - c * P2;
        const int y2 = p2 / n2, x2 = p2 - y2 * n2;
        const float *s = b0 + wi * s0 + c * P + 2 * y2 * n + 2 * x2;
        b1[wi * s1 + c * P2 + p2] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[n], s[n + 1]));
    }
    __syncthreads();
    verify_conv<16, false>(b1, s1, b0, s0, wts + L.conv_w[2], wts + L.conv_b[2], 8, m2, n2, nwin);
    __syncthreads();
    verify_conv<16, true>(b0, s0, feat + (size_t)win0 * L.F, (size_t)L.F, wts + L.conv_w[3], wts + L.conv_b[3], 16, m2, n2,
                          nwin);
}

typedef float verify_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void verify_back_kernel(const float *__restrict__ feat, int N, int F,
                                                          const float *__restrict__ w0, const float *__restrict__ bias0,
                                                          const float *__restrict__ w1, const float *__restrict__ bias1,
                                                          const float *__restrict__ scores, float *out) {
    __shared__ float sa[2][WB_VERIFY_TILE * WB_VERIFY_APITCH];
    __shared__ float sh[WB_VERIFY_TILE * WB_VERIFY_HPITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int win0 = blockIdx.x * WB_VERIFY_TILE;
    // staging: thread t carries 4 k of row t / 4 (rows behind the last window repeat it)
    const int lrow = tid >> 2, lq = tid & 3;
    const int grow = win0 + lrow < N ? win0 + lrow : N - 1;
    const float *arow = feat + (size_t)grow * F + 4 * lq;
    // v_mfma_f32_32x32x2_f32: lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31]
    const int row = lane & 31, kh = lane >> 5;
    const int col = wave * 32 + row;
    verify_f32x16 acc0, acc1;
    const float b = bias0[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = b;
    float4 nxt = *reinterpret_cast<const float4 *>(arow);
    const int stages = F / WB_VERIFY_KC;
    for (int c = 0; c < stages; ++c) {
        float *s = sa[c & 1];
        float *d = s + lrow * WB_VERIFY_APITCH + 4 * lq;
        d[0] = nxt.x, d[1] = nxt.y, d[2] = nxt.z, d[3] = nxt.w;
        // one barrier per stage: a thread that writes stage c + 2 into this buffer has passed the barrier of stage c + 1,
        // which every thread reaches only after its reads of stage c
        __syncthreads();
        if (c + 1 < stages) nxt = *reinterpret_cast<const float4 *>(arow + (c + 1) * WB_VERIFY_KC);
        const float *wk = w0 + (size_t)(c * WB_VERIFY_KC + kh) * WB_VERIFY_HIDDEN + col;
#pragma unroll
        for (int ks = 0; ks < WB_VERIFY_KC / 2; ++ks) {
            const float bv = wk[ks * 2 * WB_VERIFY_HIDDEN];
            const float a0 = s[row * WB_VERIFY_APITCH + 2 * ks + kh];
            const float a1 = s[(32 + row) * WB_VERIFY_APITCH + 2 * ks + kh];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc1, 0, 0, 0);
        }
    }
    // C/D map: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int hr = (r & 3) + 8 * (r >> 2) + 4 * kh;
        sh[hr * WB_VERIFY_HPITCH + col] = acc0[r] > 0.0f ? acc0[r] : 0.0f;
        sh[(32 + hr) * WB_VERIFY_HPITCH + col] = acc1[r] > 0.0f ? acc1[r] : 0.0f;
    }
    __syncthreads();
    if (tid < WB_VERIFY_TILE && win0 + tid < N) {
        const float *h = sh + tid * WB_VERIFY_HPITCH;
        float acc = bias1[0];
        for (int j = 0; j < WB_VERIFY_HIDDEN; ++j) acc = __builtin_fmaf(h[j], w1[j], acc);
        out[win0 + tid] = acc + scores[win0 + tid];
    }
}

}  // namespace

extern "C" int wb_verify_weights_floats(int m, int n, int C, int64_t *count) {
    WB_REQUIRE(count, "wb_verify_weights_floats: null pointer");
    VerifyLayout L;
    const int rc = verify_layout(m, n, C, &L, "wb_verify_weights_floats");
    if (rc != WB_OK) return rc;
    *count = L.count;
    return WB_OK;
}

extern "C" int wb_verify_scratch_bytes(int m, int n, int C, int64_t n_windows, size_t *bytes) {
    WB_REQUIRE(bytes, "wb_verify_scratch_bytes: null pointer");
    VerifyLayout L;
    const int rc = verify_layout(m, n, C, &L, "wb_verify_scratch_bytes");
    if (rc != WB_OK) return rc;
    WB_REQUIRE(n_windows >= 0, "wb_verify_scratch_bytes: n_windows = %lld: negative", (long long)n_windows);
    if (n_windows > WB_VERIFY_MAX_WINDOWS) {
        wb_set_error("wb_verify_scratch_bytes: %lld windows (at most %d in one call)", (long long)n_windows, WB_VERIFY_MAX_WINDOWS);
        return WB_ERR_UNSUPPORTED;
    }
    *bytes = (size_t)n_windows * (size_t)L.F * sizeof(float);
    return WB_OK;
}

extern "C" int wb_verify_launch(void *stream, const void *X, int x_dtype, int64_t n_windows, int m, int n, int C,
                                const float *weights, const float *scores_in, void *scratch, size_t scratch_bytes, float *out) {
    VerifyLayout L;
    const int rc = verify_layout(m, n, C, &L, "wb_verify_launch");
    if (rc != WB_OK) return rc;
    if (x_dtype != WB_DTYPE_U8 && x_dtype != WB_DTYPE_F32) {
        wb_set_error("wb_verify_launch: crops of dtype %d (WB_DTYPE_U8 or WB_DTYPE_F32)", x_dtype);
        return WB_ERR_UNSUPPORTED;
    }
    WB_REQUIRE(n_windows >= 0, "wb_verify_launch: n_windows = %lld: negative", (long long)n_windows);
    if (n_windows == 0) return WB_OK;
    if (n_windows > WB_VERIFY_MAX_WINDOWS) {
        wb_set_error("wb_verify_launch: %lld windows (at most %d in one call)", (long long)n_windows, WB_VERIFY_MAX_WINDOWS);
        return WB_ERR_UNSUPPORTED;
    }
    WB_REQUIRE(X && weights && scores_in && scratch && out, "wb_verify_launch: null pointer");
    WB_REQUIRE(x_dtype == WB_DTYPE_U8 || wb_aligned(X, 4), "wb_verify_launch: float32 crops must be 4-byte aligned");
    WB_REQUIRE(wb_aligned(weights, 16) && wb_aligned(scratch, 16),
               "wb_verify_launch: weights and scratch must be 16-byte aligned");
    WB_REQUIRE(wb_aligned(scores_in, 4) && wb_aligned(out, 4),
               "wb_verify_launch: scores_in and out must be 4-byte aligned");
    const size_t need = (size_t)n_windows * (size_t)L.F * sizeof(float);
    WB_REQUIRE(scratch_bytes >= need, "wb_verify_launch: scratch of %zu bytes, %zu needed (wb_verify_scratch_bytes)", scratch_bytes,
               need);
    const int N = (int)n_windows;
    const size_t lds = (size_t)L.pack * L.win_floats * sizeof(float);
    if (lds > 48 * 1024)        // (per device, and cheap: asked for on every such call)
        WB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&verify_front_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, WB_VERIFY_FRONT_LDS_MAX));
    float *feat = static_cast<float *>(scratch);
    hipLaunchKernelGGL(verify_front_kernel, dim3((uint32_t)((N + L.pack - 1) / L.pack)), dim3(256), lds, (hipStream_t)stream, X,
                       x_dtype == WB_DTYPE_U8 ? 1 : 0, N, m, n, C, L.pack, weights, L, feat);
    WB_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(verify_back_kernel, dim3((uint32_t)((N + WB_VERIFY_TILE - 1) / WB_VERIFY_TILE)), dim3(256), 0,
                       (hipStream_t)stream, feat, N, L.F, weights + L.dense0_w, weights + L.dense0_b, weights + L.dense1_w,
                       weights + L.dense1_b, scores_in, out);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
