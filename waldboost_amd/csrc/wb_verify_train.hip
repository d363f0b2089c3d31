// Training of the verification CNN (wb_verify_train_step): one step of Keras's train_on_batch for the reference's
// verification.model_cnn under its exploss and Adam (reference verification.py:28-81).  tests/verify_train_reference.py is
// the NumPy statement of the step, DESIGN section 4.11 its prose.
//
// The step (B windows picked out of a resident pool by idx, Y = -1 / +1, detector scores H):
//   * four blocks z = conv3x3_same(x, W) + bias; per channel mu and the biased variance var over the batch and all pixels;
//     xhat = (z - mu) * (1 / sqrt(var + epsilon)); y = gamma * xhat + beta; a = y > 0 ? y : 0.  2x2 max pool (floor) after
//     block 2.  Flatten in (row, column, channel) order, dropout, dense F->128, ReLU, dropout, dense 128->1, + H.
//   * e = exp(-Y p), loss = mean(clip(e, 1e-6, 1e3)), dloss/dp = -Y e / B where 1e-6 < e < 1e3 and 0 elsewhere.
//   * the backward pass by the usual rules; the pool sends its gradient to the first maximum in (row, column) order;
//     batch normalisation backward uses the batch statistics.  THE GRADIENT OF A CONVOLUTION'S BIAS IS ZERO BY CONTRACT
//     (under batch statistics it is zero in exact arithmetic): the four biases never move and take no Adam state.
//   * moving_mean = momentum * moving_mean + (1 - momentum) * mu, moving_variance likewise with var * n / (n - 1).
//   * Adam: lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) (in float64, once per workgroup), m = beta1 m + (1 - beta1) g,
//     v = beta2 v + (1 - beta2) g g, theta -= lr_t m / (sqrt(v) + epsilon), t kept on the device.
//   * dropout: inverted, an element is kept iff bits(seed, step, layer, index) >= round(rate * 2^32), kept values are
//     multiplied by float32(1 / (1 - rate)).  With fmix32(x): x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13, x *= 0xC2B2AE35,
//     x ^= x >> 16 (uint32 arithmetic):
//         key  = fmix32(seed ^ fmix32(2 * step + layer + 0x9E3779B9))        layer 0: the flat features, 1: the hidden units
//         bits = fmix32((index * 0x9E3779B1) ^ key)                          index: b * F + f, or b * 128 + j
//     step is t before the update (0 for the first step).  rate = 0 keeps everything and multiplies by 1: the identity.
//
// Determinism: every sum has a fixed order.  Per-channel sums and weight gradients are taken per workgroup over a fixed
// range (a fixed tree inside the workgroup), written as partials and combined in ascending workgroup order; no
// floating-point atomics; the one integer atomic counts the update kernel's workgroups so that the last one advances t,
// which changes who writes t, never what is written.  Bit parity with a NumPy statement is NOT claimed (unlike
// wb_verify_launch): plain float32 with fmaf where written, against a float64 statement within a measured margin.
//
// The step is a chain of launches on one stream over a caller-provided scratch.  Activations are [window][pixel][channel]
// in global memory; a thread of the convolution kernel owns one pixel and all its output channels, and the weights of a
// step are the same address in every lane (scalar loads).  Backward-data is the same routine with the kernel flipped and
// its channel axes swapped.  Every value read from the scratch is written earlier in the same step.
#include "wb_common.h"
#include <math.h>

#define VT_MAX_SIDE 32
#define VT_MAX_C 16
#define VT_HIDDEN 128
#define VT_MAX_BATCH 1024
#define VT_MAX_PART 128         // most partials of one fixed-order sum
#define VT_ROWS_PER_PART 256    // rows of [row][channel] one workgroup of a per-channel sum takes (at least)
#define VT_WGRAD_THREADS 1024    // threads of a weight-gradient workgroup

namespace {

struct VtLayout {
    int m, n, C, m2, n2, P, P2, F;
    int64_t off[29];            // the 28 arrays of the training layout, then their total
};

struct VtSegments {
    int64_t off[29];
};

int vt_layout(int m, int n, int C, VtLayout *L, const char *who) {
    if (m < 2 || n < 2 || m > VT_MAX_SIDE || n > VT_MAX_SIDE || C < 1 || C > VT_MAX_C) {
        wb_set_error("%s: window shape (%d, %d, %d): supported are 2 <= m, n <= %d and 1 <= C <= %d", who, m, n, C, VT_MAX_SIDE,
                     VT_MAX_C);
        return WB_ERR_UNSUPPORTED;
    }
    L->m = m, L->n = n, L->C = C, L->m2 = m / 2, L->n2 = n / 2, L->P = m * n, L->P2 = L->m2 * L->n2, L->F = L->P2 * 16;
    const int cin[4] = {C, 8, 8, 16}, cout[4] = {8, 8, 16, 16};
    int64_t at = 0;
    for (int k = 0; k < 4; ++k) {
        L->off[6 * k] = at, at += 9 * cin[k] * cout[k];
        for (int r = 1; r < 6; ++r) L->off[6 * k + r] = at, at += cout[k];
    }
    L->off[24] = at, at += (int64_t)L->F * VT_HIDDEN;
    L->off[25] = at, at += VT_HIDDEN;
    L->off[26] = at, at += VT_HIDDEN;
    L->off[27] = at, at += 1;
    L->off[28] = at;
    return WB_OK;
}

int vt_check_batch(int64_t B, const char *who) {
    if (B < 2 || B > VT_MAX_BATCH || (B & 1)) {
        wb_set_error("%s: batch of %lld windows: supported are even sizes 2 .. %d", who, (long long)B, VT_MAX_BATCH);
        return WB_ERR_UNSUPPORTED;
    }
    return WB_OK;
}

// floats of the scratch, each buffer a multiple of 4 floats
struct VtScratch {
    size_t z[4], a[4], a2p, a4d, hd, du, bufA, bufB, part_fwd, stats, part_bwd, wpart, grad, total;
    int G1, G2, GW;             // workgroups of the per-channel sums (full size, pooled size) and of the weight gradients
};

size_t vt_round4(size_t x) { return (x + 3) & ~(size_t)3; }

int vt_parts(size_t rows) {
    size_t g = (rows + VT_ROWS_PER_PART - 1) / VT_ROWS_PER_PART;
    return g > VT_MAX_PART ? VT_MAX_PART : (int)g;
}

void vt_scratch(const VtLayout &L, int B, VtScratch *S) {
    const size_t n1 = (size_t)B * L.P, n2 = (size_t)B * L.P2;
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t here = at; at += vt_round4(floats); return here; };
    S->z[0] = take(n1 * 8), S->a[0] = take(n1 * 8), S->z[1] = take(n1 * 8), S->a[1] = take(n1 * 8);
    S->a2p = take(n2 * 8);
    S->z[2] = take(n2 * 16), S->a[2] = take(n2 * 16), S->z[3] = take(n2 * 16), S->a[3] = take(n2 * 16);
    S->a4d = take(n2 * 16);
    S->hd = take((size_t)B * VT_HIDDEN), S->du = take((size_t)B * VT_HIDDEN);
    S->bufA = take(n1 * 8), S->bufB = take(n1 * 8);              // (n2 * 16 <= n1 * 4)
    S->part_fwd = take((size_t)2 * VT_MAX_PART * 16);
    S->stats = take((size_t)4 * 32);                              // per block: mu [16], 1 / sqrt(var + epsilon) [16]
    S->part_bwd = take((size_t)2 * VT_MAX_PART * 16);
    S->wpart = take((size_t)VT_MAX_PART * 9 * 16 * 16);
    S->grad = take((size_t)L.off[28]);
    S->total = at;
    S->G1 = vt_parts(n1), S->G2 = vt_parts(n2);
    S->GW = B < VT_MAX_PART ? B : VT_MAX_PART;
}

__device__ inline uint32_t vt_fmix32(uint32_t x) {
    x ^= x >> 16, x *= 0x85EBCA6Bu, x ^= x >> 13, x *= 0xC2B2AE35u, x ^= x >> 16;
    return x;
}
__device__ inline uint32_t vt_drop_key(uint32_t seed, uint32_t step, uint32_t layer) {
    return vt_fmix32(seed ^ vt_fmix32(2u * step + layer + 0x9E3779B9u));
}
__device__ inline bool vt_keep(uint32_t key, uint32_t index, uint32_t threshold) {
    return vt_fmix32((index * 0x9E3779B1u) ^ key) >= threshold;
}

__device__ inline int vt_window(const int32_t *idx, int b, int n_pool) {
    const int w = idx[b];
    return w < 0 ? 0 : (w >= n_pool ? n_pool - 1 : w);          // (the caller checks its indices; nothing is read outside the pool)
}

// MODE of a convolution's input: a float buffer [B][pixel][cin], or the pool's windows picked by idx
enum { VT_IN_BUFFER = 0, VT_IN_POOL_U8 = 1, VT_IN_POOL_F32 = 2 };

template <int MODE>
__device__ inline float vt_load(const void *in, size_t at) {
    return MODE == VT_IN_POOL_U8 ? (float)static_cast<const uint8_t *>(in)[at] : static_cast<const float *>(in)[at];
}

// out[b][p][o] = bias[o] + sum over (ky, kx, i), in this order, of in[b][p + (ky - 1, kx - 1)][i] * w(ky, kx, i, o); taps
// outside the window are multiplied by zero.  Forward: w = W[ky][kx][i][o].  BACKWARD (the gradient of the input from the
// gradient of the output): w = W[2 - ky][2 - kx][o][i] of the forward kernel W[3][3][COUT][cin], and no bias.
template <int COUT, int MODE, bool BACKWARD>
__global__ __launch_bounds__(256) void vt_conv_kernel(const void *in, const int32_t *idx, int n_pool, int B, int H, int W, int cin,
                                                      const float *__restrict__ w, const float *__restrict__ bias, float *out) {
    const int P = H * W;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= B * P) return;
    const int b = item / P, p = item - b * P;
    const int y = p / W, x = p - y * W;
    const size_t base = (size_t)(MODE == VT_IN_BUFFER ? b : vt_window(idx, b, n_pool)) * P * cin;
    float acc[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[o] = BACKWARD ? 0.0f : bias[o];
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll 1
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            const bool inside = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const size_t at = base + (size_t)(inside ? yy * W + xx : p) * cin;
            const float *wt = BACKWARD ? w + ((2 - ky) * 3 + (2 - kx)) * COUT * cin : w + (ky * 3 + kx) * cin * COUT;
#pragma unroll 2
            for (int i = 0; i < cin; ++i) {
                float v = vt_load<MODE>(in, at + i);          // (always read: the clamped address is inside the window)
                v = inside ? v : 0.0f;
#pragma unroll
                for (int o = 0; o < COUT; ++o) acc[o] = __builtin_fmaf(v, BACKWARD ? wt[o * cin + i] : wt[i * COUT + o], acc[o]);
            }
        }
    }
    float4 *dst = reinterpret_cast<float4 *>(out + (size_t)item * COUT);
#pragma unroll
    for (int o = 0; o < COUT; o += 4) dst[o / 4] = make_float4(acc[o], acc[o + 1], acc[o + 2], acc[o + 3]);
}

// ---- per-channel sums over [rows][C], C = 8 or 16: thread t takes channel t % C of rows r0 + t / C, + 256 / C, ... of its
// workgroup's range; the 256 / C values of a channel are added by a fixed tree; sh[c] holds the sum
__device__ inline void vt_tree(float *sh, float v, int C) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s >= C; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
}
// partials [G][16] added in ascending workgroup order
__device__ inline float vt_combine(const float *part, int G, int c) {
    float acc = 0.0f;
    for (int g = 0; g < G; ++g) acc += part[g * 16 + c];
    return acc;
}

__global__ __launch_bounds__(256) void vt_bn_mean_part(const float *z, int rows, int C, int rows_per, float *part) {
    __shared__ float sh[256];
    const int c = threadIdx.x % C, R = 256 / C;
    const int r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    float acc = 0.0f;
    for (int r = r0 + threadIdx.x / C; r < r1; r += R) acc += z[(size_t)r * C + c];
    vt_tree(sh, acc, C);
    if ((int)threadIdx.x < C) part[blockIdx.x * 16 + threadIdx.x] = sh[threadIdx.x];
}

__global__ __launch_bounds__(256) void vt_bn_var_part(const float *z, int rows, int C, int rows_per, const float *mean_part, int G,
                                                      float *part) {
    __shared__ float sh[256];
    __shared__ float mu[16];
    if ((int)threadIdx.x < C) mu[threadIdx.x] = vt_combine(mean_part, G, threadIdx.x) / (float)rows;
    __syncthreads();
    const int c = threadIdx.x % C, R = 256 / C;
    const int r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    float acc = 0.0f;
    for (int r = r0 + threadIdx.x / C; r < r1; r += R) {
        const float d = z[(size_t)r * C + c] - mu[c];
        acc = __builtin_fmaf(d, d, acc);
    }
    vt_tree(sh, acc, C);
    if ((int)threadIdx.x < C) part[blockIdx.x * 16 + threadIdx.x] = sh[threadIdx.x];
}

// a = relu(gamma * xhat + beta); workgroup 0 also keeps mu and 1 / sqrt(var + epsilon) for the backward pass and hands mu and
// the unbiased variance to the update (the moving-statistics slots of the gradient buffer)
__global__ __launch_bounds__(256) void vt_bn_apply(const float *z, int rows, int C, const float *mean_part, const float *var_part,
                                                   int G, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                   float epsilon, float *a, float *stats, float *stat_mean, float *stat_var) {
    __shared__ float mu[16], inv[16];
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const float mean = vt_combine(mean_part, G, c) / (float)rows;
        const float var = vt_combine(var_part, G, c) / (float)rows;
        mu[c] = mean, inv[c] = 1.0f / sqrtf(var + epsilon);
        if (blockIdx.x == 0) {
            stats[c] = mean, stats[16 + c] = inv[c];
            stat_mean[c] = mean, stat_var[c] = var * ((float)rows / (float)(rows - 1));
        }
    }
    __syncthreads();
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)rows * C) return;
    const int c = (int)(e % C);
    const float xhat = (z[e] - mu[c]) * inv[c];
    const float y = gamma[c] * xhat + beta[c];
    a[e] = y > 0.0f ? y : 0.0f;
}

// sums of dy and dy * xhat per channel, dy = da where the block's output is positive
__global__ __launch_bounds__(256) void vt_bn_bwd_part(const float *da, const float *a, const float *z, const float *stats, int rows,
                                                      int C, int rows_per, float *part) {
    __shared__ float sh[256];
    const int c = threadIdx.x % C, R = 256 / C;
    const int r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    const float mu = stats[c], inv = stats[16 + c];
    float s0 = 0.0f, s1 = 0.0f;
    for (int r = r0 + threadIdx.x / C; r < r1; r += R) {
        const size_t e = (size_t)r * C + c;
        const float dy = a[e] > 0.0f ? da[e] : 0.0f;
        s0 += dy;
        s1 = __builtin_fmaf(dy, (z[e] - mu) * inv, s1);
    }
    vt_tree(sh, s0, C);
    if ((int)threadIdx.x < C) part[blockIdx.x * 16 + threadIdx.x] = sh[threadIdx.x];
    __syncthreads();
    vt_tree(sh, s1, C);
    if ((int)threadIdx.x < C) part[(VT_MAX_PART + blockIdx.x) * 16 + threadIdx.x] = sh[threadIdx.x];
}

// dz = gamma / sqrt(var + epsilon) * (dy - dbeta / n - xhat * dgamma / n); workgroup 0 writes dgamma and dbeta
__global__ __launch_bounds__(256) void vt_bn_bwd_apply(const float *da, const float *a, const float *z, const float *stats, int rows,
                                                       int C, const float *part, int G, const float *__restrict__ gamma, float *dz,
                                                       float *dgamma, float *dbeta) {
    __shared__ float sb[16], sg[16];
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        sb[c] = vt_combine(part, G, c), sg[c] = vt_combine(part + VT_MAX_PART * 16, G, c);
        if (blockIdx.x == 0) dbeta[c] = sb[c], dgamma[c] = sg[c];
    }
    __syncthreads();
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)rows * C) return;
    const int c = (int)(e % C);
    const float inv = stats[16 + c], xhat = (z[e] - stats[c]) * inv;
    const float dy = a[e] > 0.0f ? da[e] : 0.0f;
    const float nf = (float)rows;
    dz[e] = gamma[c] * inv * (dy - sb[c] / nf - xhat * (sg[c] / nf));
}

// 2x2 maximum, 8 channels, the last row / column of an odd size dropped
__global__ __launch_bounds__(256) void vt_pool_fwd(const float *a, int B, int m, int n, float *out) {
    const int m2 = m >> 1, n2 = n >> 1;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * m2 * n2 * 8) return;
    const int c = e & 7, q = e >> 3;
    const int b = q / (m2 * n2), p2 = q - b * (m2 * n2);
    const int y2 = p2 / n2, x2 = p2 - y2 * n2;
    const float *s = a + ((size_t)b * m * n + (size_t)2 * y2 * n + 2 * x2) * 8 + c;
    float best = s[0];
    best = s[8] > best ? s[8] : best;
    best = s[(size_t)n * 8] > best ? s[(size_t)n * 8] : best;
    best = s[(size_t)n * 8 + 8] > best ? s[(size_t)n * 8 + 8] : best;
    out[e] = best;
}

// the pooled gradient goes to the first maximum in (row, column) order, zero to everything else
__global__ __launch_bounds__(256) void vt_pool_bwd(const float *dpool, const float *a, int B, int m, int n, float *da) {
    const int m2 = m >> 1, n2 = n >> 1;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * m * n * 8) return;
    const int c = e & 7, q = e >> 3;
    const int b = q / (m * n), p = q - b * (m * n);
    const int y = p / n, x = p - y * n;
    float g = 0.0f;
    if (y < 2 * m2 && x < 2 * n2) {
        const int y2 = y >> 1, x2 = x >> 1;
        const float *s = a + ((size_t)b * m * n + (size_t)2 * y2 * n + 2 * x2) * 8 + c;
        float best = s[0];
        int k = 0;
        if (s[8] > best) best = s[8], k = 1;
        if (s[(size_t)n * 8] > best) best = s[(size_t)n * 8], k = 2;
        if (s[(size_t)n * 8 + 8] > best) k = 3;
        if (k == (y & 1) * 2 + (x & 1)) g = dpool[((size_t)b * m2 * n2 + (size_t)y2 * n2 + x2) * 8 + c];
    }
    da[e] = g;
}

// dW[ky][kx][i][o] = sum over windows and pixels of in[b][p + (ky - 1, kx - 1)][i] * dz[b][p][o].  Workgroup g takes
// windows g * B / G .. (g + 1) * B / G; a thread owns one (i, o) and nine sums; the (window, pixel) items are dealt to
// VT_WGRAD_THREADS / (cin * cout) threads per (i, o), whose sums are then added in ascending order.
template <int MODE>
__global__ __launch_bounds__(VT_WGRAD_THREADS) void vt_wgrad_part(const void *in, const int32_t *idx, int n_pool, const float *dz, int B, int H,
                                                     int W, int cin, int cout, float *part) {
    __shared__ float sh[9 * VT_WGRAD_THREADS];
    const int P = H * W, pairs = cin * cout, sub = VT_WGRAD_THREADS / pairs;
    const int s = threadIdx.x / pairs, pr = threadIdx.x - s * pairs;
    const int i = pr / cout, o = pr - i * cout;
    const int b0 = (int)((int64_t)blockIdx.x * B / gridDim.x), b1 = (int)((int64_t)(blockIdx.x + 1) * B / gridDim.x);
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0f;
    if (s < sub) {
        for (int q = s; q < (b1 - b0) * P; q += sub) {
            const int b = b0 + q / P, p = q % P;
            const int y = p / W, x = p - y * W;
            const size_t base = (size_t)(MODE == VT_IN_BUFFER ? b : vt_window(idx, b, n_pool)) * P * cin + i;
            const float d = dz[((size_t)b * P + p) * cout + o];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
                const bool inside = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                float v = vt_load<MODE>(in, base + (size_t)(inside ? yy * W + xx : p) * cin);
                v = inside ? v : 0.0f;
                acc[k] = __builtin_fmaf(v, d, acc[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) sh[k * VT_WGRAD_THREADS + threadIdx.x] = acc[k];
    __syncthreads();
    if (s == 0) {
        for (int k = 0; k < 9; ++k) {
            float total = 0.0f;
            for (int j = 0; j < sub; ++j) total += sh[k * VT_WGRAD_THREADS + j * pairs + pr];
            part[(size_t)blockIdx.x * 9 * pairs + (size_t)k * pairs + pr] = total;
        }
    }
}

__global__ __launch_bounds__(256) void vt_sum_parts(const float *part, int G, int count, float *out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    float acc = 0.0f;
    for (int g = 0; g < G; ++g) acc += part[(size_t)g * count + j];
    out[j] = acc;
}

__global__ __launch_bounds__(256) void vt_dropout_fwd(const float *a, int count, uint32_t seed, const int32_t *t, uint32_t threshold,
                                                      float scale, float *out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const uint32_t key = vt_drop_key(seed, (uint32_t)t[0], 0u);
    out[e] = vt_keep(key, (uint32_t)e, threshold) ? a[e] * scale : 0.0f;
}

// hd[b][j] = dropout(relu(u)), u = b0[j] + the four quarter sums over k (each k ascending from 0), added in ascending order.
// A workgroup takes one window and 64 hidden units; wave q takes the k of quarter q.
__global__ __launch_bounds__(256) void vt_dense0_fwd(const float *x, const float *__restrict__ W0, const float *__restrict__ b0, int B,
                                                     int F, uint32_t seed, const int32_t *t, uint32_t threshold, float scale,
                                                     float *hd) {
    __shared__ float sh[256];
    const int b = blockIdx.x >> 1, j = (blockIdx.x & 1) * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const int quarter = F >> 2;                         // (F is a multiple of 16)
    const float *row = x + (size_t)b * F + (size_t)q * quarter;
    const float *col = W0 + (size_t)q * quarter * VT_HIDDEN + j;
    float acc = 0.0f;
#pragma unroll 4
    for (int k = 0; k < quarter; ++k) acc = __builtin_fmaf(row[k], col[(size_t)k * VT_HIDDEN], acc);
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    float u = b0[j];
    u += sh[threadIdx.x], u += sh[64 + threadIdx.x], u += sh[128 + threadIdx.x], u += sh[192 + threadIdx.x];
    u = u > 0.0f ? u : 0.0f;
    const uint32_t e = (uint32_t)(b * VT_HIDDEN + j);
    const uint32_t key = vt_drop_key(seed, (uint32_t)t[0], 1u);
    hd[e] = vt_keep(key, e, threshold) ? u * scale : 0.0f;
}

// One workgroup: p = b1 + sum hd w1 + H, the loss and its mean (a fixed tree over 1024 slots), dloss/dp, the gradients of
// the last layer, du = the gradient at the hidden pre-activations, and the gradient of the hidden bias.
__global__ __launch_bounds__(256) void vt_head_kernel(const float *hd, const float *__restrict__ w1, const float *__restrict__ b1,
                                                      const float *Hs, const float *Ys, const int32_t *idx, int n_pool, int B,
                                                      float scale, float *du, float *g_w1, float *g_b1, float *g_b0,
                                                      float *loss_out) {
    __shared__ float sl[VT_MAX_BATCH], sdp[VT_MAX_BATCH];
    const int tid = threadIdx.x;
    for (int b = tid; b < VT_MAX_BATCH; b += 256) {
        float l = 0.0f, d = 0.0f;
        if (b < B) {
            float p = b1[0];
            for (int j = 0; j < VT_HIDDEN; ++j) p = __builtin_fmaf(hd[(size_t)b * VT_HIDDEN + j], w1[j], p);
            const int w = vt_window(idx, b, n_pool);
            p += Hs[w];
            const float y = Ys[w];
            const float e = expf(-y * p);
            l = fminf(fmaxf(e, 1e-6f), 1e3f);
            d = (e > 1e-6f && e < 1e3f) ? -y * e / (float)B : 0.0f;
        }
        sl[b] = l, sdp[b] = d;
    }
    __syncthreads();
    for (int e = tid; e < B * VT_HIDDEN; e += 256)
        du[e] = hd[e] > 0.0f ? sdp[e >> 7] * w1[e & (VT_HIDDEN - 1)] * scale : 0.0f;
    for (int s = VT_MAX_BATCH / 2; s >= 1; s >>= 1) {
        for (int k = tid; k < s; k += 256) sl[k] += sl[k + s];
        __syncthreads();
    }
    if (tid < VT_HIDDEN) {
        float gw = 0.0f, gb = 0.0f;
        for (int b = 0; b < B; ++b) {
            gw = __builtin_fmaf(hd[(size_t)b * VT_HIDDEN + tid], sdp[b], gw);
            gb += du[(size_t)b * VT_HIDDEN + tid];        // (written by this workgroup before the barriers above)
        }
        g_w1[tid] = gw, g_b0[tid] = gb;
    }
    if (tid == VT_HIDDEN) {
        float gb = 0.0f;
        for (int b = 0; b < B; ++b) gb += sdp[b];
        g_b1[0] = gb;
        loss_out[0] = sl[0] / (float)B;
    }
}

// dW0[f][j] = sum over b ascending of x[b][f] * du[b][j]
__global__ __launch_bounds__(256) void vt_dense0_bwd_w(const float *x, const float *du, int B, int F, float *g_w0) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= F * VT_HIDDEN) return;
    const int f = e >> 7, j = e & (VT_HIDDEN - 1);
    float acc = 0.0f;
    for (int b = 0; b < B; ++b) acc = __builtin_fmaf(x[(size_t)b * F + f], du[(size_t)b * VT_HIDDEN + j], acc);
    g_w0[e] = acc;
}

// da[b][f] = dropout'(sum over j ascending of du[b][j] * W0[f][j])
__global__ __launch_bounds__(256) void vt_dense0_bwd_x(const float *du, const float *__restrict__ W0, int B, int F, uint32_t seed,
                                                       const int32_t *t, uint32_t threshold, float scale, float *da) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * F) return;
    const int b = e / F, f = e - b * F;
    const float4 *d4 = reinterpret_cast<const float4 *>(du + (size_t)b * VT_HIDDEN);
    const float4 *w4 = reinterpret_cast<const float4 *>(W0 + (size_t)f * VT_HIDDEN);
    float acc = 0.0f;
#pragma unroll 4
    for (int j = 0; j < VT_HIDDEN / 4; ++j) {
        const float4 d = d4[j], w = w4[j];
        acc = __builtin_fmaf(d.x, w.x, acc), acc = __builtin_fmaf(d.y, w.y, acc);
        acc = __builtin_fmaf(d.z, w.z, acc), acc = __builtin_fmaf(d.w, w.w, acc);
    }
    const uint32_t key = vt_drop_key(seed, (uint32_t)t[0], 0u);
    da[e] = vt_keep(key, (uint32_t)e, threshold) ? acc * scale : 0.0f;
}

struct VtAdam {
    double lr, beta1, beta2;
    float b1, b2, epsilon, momentum;
};

// One thread per parameter of the training layout.  Kernels, gamma, beta and the dense layers take an Adam step; the
// convolution biases stay (their gradient is zero by contract); the moving statistics follow the step's statistics.
// t[0] is the number of steps done, t[1] counts the workgroups that have finished: the last one advances t[0] and puts
// t[1] back to zero.
__global__ __launch_bounds__(256) void vt_update_kernel(float *params, float *adam_m, float *adam_v, int32_t *t, const float *grad,
                                                        float *grads_out, VtSegments seg, VtAdam h) {
    __shared__ float lr_t;
    if (threadIdx.x == 0) {
        const double step = (double)(t[0] + 1);
        lr_t = (float)(h.lr * sqrt(1.0 - pow(h.beta2, step)) / (1.0 - pow(h.beta1, step)));
    }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < seg.off[28]) {
        int s = 0;              // the array e lies in (the offsets stay in scalar registers: no indexing by a lane's value)
#pragma unroll
        for (int k = 1; k < 28; ++k) s += e >= seg.off[k] ? 1 : 0;
        const int r = s < 24 ? s % 6 : 0;       // 0 kernel, 1 bias, 2 gamma, 3 beta, 4 moving_mean, 5 moving_variance
        if (s < 24 && r == 1) {
            if (grads_out) grads_out[e] = 0.0f;
        } else if (s < 24 && r >= 4) {
            const float stat = grad[e];
            params[e] = h.momentum * params[e] + (1.0f - h.momentum) * stat;
            if (grads_out) grads_out[e] = stat;
        } else {
            const float g = grad[e];
            const float m = h.b1 * adam_m[e] + (1.0f - h.b1) * g;
            const float v = h.b2 * adam_v[e] + (1.0f - h.b2) * (g * g);
            adam_m[e] = m, adam_v[e] = v;
            params[e] = params[e] - lr_t * m / (sqrtf(v) + h.epsilon);
            if (grads_out) grads_out[e] = g;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&t[1], 1) == (int)gridDim.x - 1) {
            t[1] = 0;
            t[0] = t[0] + 1;
        }
    }
}

inline uint32_t vt_blocks(size_t items) { return (uint32_t)((items + 255) / 256); }

template <int COUT, bool BACKWARD>
void vt_conv(hipStream_t st, int mode, const void *in, const int32_t *idx, int n_pool, int B, int H, int W, int cin, const float *w,
             const float *bias, float *out) {
    const dim3 grid(vt_blocks((size_t)B * H * W)), block(256);
    if (mode == VT_IN_POOL_U8)
        hipLaunchKernelGGL((vt_conv_kernel<COUT, VT_IN_POOL_U8, BACKWARD>), grid, block, 0, st, in, idx, n_pool, B, H, W, cin, w, bias, out);
    else if (mode == VT_IN_POOL_F32)
        hipLaunchKernelGGL((vt_conv_kernel<COUT, VT_IN_POOL_F32, BACKWARD>), grid, block, 0, st, in, idx, n_pool, B, H, W, cin, w, bias, out);
    else
        hipLaunchKernelGGL((vt_conv_kernel<COUT, VT_IN_BUFFER, BACKWARD>), grid, block, 0, st, in, idx, n_pool, B, H, W, cin, w, bias, out);
}

void vt_wgrad(hipStream_t st, int mode, const void *in, const int32_t *idx, int n_pool, const float *dz, int B, int H, int W, int cin,
              int cout, int G, float *part, float *out) {
    const dim3 grid(G), block(VT_WGRAD_THREADS);
    if (mode == VT_IN_POOL_U8)
        hipLaunchKernelGGL(vt_wgrad_part<VT_IN_POOL_U8>, grid, block, 0, st, in, idx, n_pool, dz, B, H, W, cin, cout, part);
    else if (mode == VT_IN_POOL_F32)
        hipLaunchKernelGGL(vt_wgrad_part<VT_IN_POOL_F32>, grid, block, 0, st, in, idx, n_pool, dz, B, H, W, cin, cout, part);
    else
        hipLaunchKernelGGL(vt_wgrad_part<VT_IN_BUFFER>, grid, block, 0, st, in, idx, n_pool, dz, B, H, W, cin, cout, part);
    const int count = 9 * cin * cout;
    hipLaunchKernelGGL(vt_sum_parts, dim3(vt_blocks(count)), dim3(256), 0, st, part, G, count, out);
}

}  // namespace

extern "C" int wb_verify_train_param_floats(int m, int n, int C, int64_t *count) {
    WB_REQUIRE(count, "wb_verify_train_param_floats: null pointer");
    VtLayout L;
    const int rc = vt_layout(m, n, C, &L, "wb_verify_train_param_floats");
    if (rc != WB_OK) return rc;
    *count = L.off[28];
    return WB_OK;
}

extern "C" int wb_verify_train_scratch_bytes(int m, int n, int C, int64_t batch, size_t *bytes) {
    WB_REQUIRE(bytes, "wb_verify_train_scratch_bytes: null pointer");
    VtLayout L;
    int rc = vt_layout(m, n, C, &L, "wb_verify_train_scratch_bytes");
    if (rc != WB_OK) return rc;
    rc = vt_check_batch(batch, "wb_verify_train_scratch_bytes");
    if (rc != WB_OK) return rc;
    VtScratch S;
    vt_scratch(L, (int)batch, &S);
    *bytes = S.total * sizeof(float);
    return WB_OK;
}

extern "C" int wb_verify_train_step(void *stream, const void *X, int x_dtype, const float *H, const float *Y, int64_t n_pool,
                                    const int32_t *idx, int64_t batch, int m, int n, int C, float *params, float *adam_m,
                                    float *adam_v, int32_t *t, const WbVerifyTrainHyper *hyper, void *scratch, size_t scratch_bytes,
                                    float *loss_out, float *grads_out) {
    const char *who = "wb_verify_train_step";
    VtLayout L;
    int rc = vt_layout(m, n, C, &L, who);
    if (rc != WB_OK) return rc;
    if (x_dtype != WB_DTYPE_U8 && x_dtype != WB_DTYPE_F32) {
        wb_set_error("%s: crops of dtype %d (WB_DTYPE_U8 or WB_DTYPE_F32)", who, x_dtype);
        return WB_ERR_UNSUPPORTED;
    }
    rc = vt_check_batch(batch, who);
    if (rc != WB_OK) return rc;
    WB_REQUIRE(n_pool >= 1 && n_pool <= INT32_MAX, "%s: a pool of %lld windows", who, (long long)n_pool);
    WB_REQUIRE(X && H && Y && idx && params && adam_m && adam_v && t && hyper && scratch && loss_out, "%s: null pointer", who);
    WB_REQUIRE(x_dtype == WB_DTYPE_U8 || wb_aligned(X, 4), "%s: float32 crops must be 4-byte aligned", who);
    WB_REQUIRE(wb_aligned(params, 16) && wb_aligned(adam_m, 16) && wb_aligned(adam_v, 16) && wb_aligned(scratch, 16),
               "%s: params, adam_m, adam_v and scratch must be 16-byte aligned", who);
    WB_REQUIRE(wb_aligned(H, 4) && wb_aligned(Y, 4) && wb_aligned(idx, 4) && wb_aligned(t, 4) && wb_aligned(loss_out, 4) && wb_aligned(grads_out, 4),
               "%s: H, Y, idx, t, loss_out and grads_out must be 4-byte aligned", who);
    const WbVerifyTrainHyper &hy = *hyper;
    WB_REQUIRE(hy.lr >= 0.0 && hy.lr < 1e30 && hy.beta1 >= 0.0 && hy.beta1 < 1.0 && hy.beta2 >= 0.0 && hy.beta2 < 1.0 &&
                   hy.adam_epsilon > 0.0 && hy.adam_epsilon < 1e30 && hy.momentum >= 0.0 && hy.momentum <= 1.0 &&
                   hy.bn_epsilon > 0.0 && hy.bn_epsilon < 1e30 && hy.dropout >= 0.0 && hy.dropout < 1.0,
               "%s: hyper: lr >= 0, 0 <= beta < 1, epsilons > 0, 0 <= momentum <= 1 and 0 <= dropout < 1 are required", who);
    const int B = (int)batch;
    VtScratch S;
    vt_scratch(L, B, &S);
    WB_REQUIRE(scratch_bytes >= S.total * sizeof(float), "%s: scratch of %zu bytes, %zu needed (wb_verify_train_scratch_bytes)", who,
               scratch_bytes, S.total * sizeof(float));

    hipStream_t st = (hipStream_t)stream;
    float *sc = static_cast<float *>(scratch);
    float *grad = sc + S.grad, *bufA = sc + S.bufA, *bufB = sc + S.bufB;
    float *part_fwd = sc + S.part_fwd, *part_bwd = sc + S.part_bwd, *wpart = sc + S.wpart;
    const int pool_mode = x_dtype == WB_DTYPE_U8 ? VT_IN_POOL_U8 : VT_IN_POOL_F32;
    const int np = (int)n_pool;
    const int cin[4] = {C, 8, 8, 16}, cout[4] = {8, 8, 16, 16};
    const int Hk[4] = {m, m, L.m2, L.m2}, Wk[4] = {n, n, L.n2, L.n2};
    const uint32_t threshold = (uint32_t)llround(hy.dropout * 4294967296.0);
    const float scale = (float)(1.0 / (1.0 - hy.dropout));
    const float bn_eps = (float)hy.bn_epsilon;
    const dim3 block(256);

    // ---- forward
    const void *layer_in[4] = {X, sc + S.a[0], sc + S.a2p, sc + S.a[2]};
    for (int k = 0; k < 4; ++k) {
        const int mode = k == 0 ? pool_mode : VT_IN_BUFFER;
        float *z = sc + S.z[k], *a = sc + S.a[k];
        const float *w = params + L.off[6 * k], *bias = params + L.off[6 * k + 1];
        if (cout[k] == 8)
            vt_conv<8, false>(st, mode, layer_in[k], idx, np, B, Hk[k], Wk[k], cin[k], w, bias, z);
        else
            vt_conv<16, false>(st, mode, layer_in[k], idx, np, B, Hk[k], Wk[k], cin[k], w, bias, z);
        const int rows = B * Hk[k] * Wk[k], G = k < 2 ? S.G1 : S.G2;
        const int rows_per = (rows + G - 1) / G;
        hipLaunchKernelGGL(vt_bn_mean_part, dim3(G), block, 0, st, z, rows, cout[k], rows_per, part_fwd);
        hipLaunchKernelGGL(vt_bn_var_part, dim3(G), block, 0, st, z, rows, cout[k], rows_per, part_fwd, G, part_fwd + VT_MAX_PART * 16);
        hipLaunchKernelGGL(vt_bn_apply, dim3(vt_blocks((size_t)rows * cout[k])), block, 0, st, z, rows, cout[k], part_fwd,
                           part_fwd + VT_MAX_PART * 16, G, params + L.off[6 * k + 2], params + L.off[6 * k + 3], bn_eps, a,
                           sc + S.stats + 32 * k, grad + L.off[6 * k + 4], grad + L.off[6 * k + 5]);
        if (k == 1)
            hipLaunchKernelGGL(vt_pool_fwd, dim3(vt_blocks((size_t)B * L.P2 * 8)), block, 0, st, a, B, m, n, sc + S.a2p);
    }
    const int BF = B * L.F;
    hipLaunchKernelGGL(vt_dropout_fwd, dim3(vt_blocks(BF)), block, 0, st, sc + S.a[3], BF, hy.seed, t, threshold, scale, sc + S.a4d);
    hipLaunchKernelGGL(vt_dense0_fwd, dim3(2 * B), block, 0, st, sc + S.a4d, params + L.off[24],
                       params + L.off[25], B, L.F, hy.seed, t, threshold, scale, sc + S.hd);
    hipLaunchKernelGGL(vt_head_kernel, dim3(1), block, 0, st, sc + S.hd, params + L.off[26], params + L.off[27], H, Y, idx, np, B, scale,
                       sc + S.du, grad + L.off[26], grad + L.off[27], grad + L.off[25], loss_out);
    WB_HIP_CHECK(hipGetLastError());

    // ---- backward
    hipLaunchKernelGGL(vt_dense0_bwd_w, dim3(vt_blocks((size_t)L.F * VT_HIDDEN)), block, 0, st, sc + S.a4d, sc + S.du, B, L.F,
                       grad + L.off[24]);
    hipLaunchKernelGGL(vt_dense0_bwd_x, dim3(vt_blocks(BF)), block, 0, st, sc + S.du, params + L.off[24], B, L.F, hy.seed, t, threshold,
                       scale, bufA);
    // the gradient of a block's output is in `da`; dz goes to the other buffer, the gradient of the block's input back to
    // the first (block 2 -> pool: one more hop)
    float *da = bufA, *other = bufB;
    for (int k = 3; k >= 0; --k) {
        const int rows = B * Hk[k] * Wk[k], G = k < 2 ? S.G1 : S.G2;
        const int rows_per = (rows + G - 1) / G;
        const float *z = sc + S.z[k], *a = sc + S.a[k], *stats = sc + S.stats + 32 * k;
        float *dz = other;
        hipLaunchKernelGGL(vt_bn_bwd_part, dim3(G), block, 0, st, da, a, z, stats, rows, cout[k], rows_per, part_bwd);
        hipLaunchKernelGGL(vt_bn_bwd_apply, dim3(vt_blocks((size_t)rows * cout[k])), block, 0, st, da, a, z, stats, rows, cout[k],
                           part_bwd, G, params + L.off[6 * k + 2], dz, grad + L.off[6 * k + 2], grad + L.off[6 * k + 3]);
        vt_wgrad(st, k == 0 ? pool_mode : VT_IN_BUFFER, layer_in[k], idx, np, dz, B, Hk[k], Wk[k], cin[k], cout[k], S.GW, wpart,
                 grad + L.off[6 * k]);
        if (k == 0) break;
        const float *w = params + L.off[6 * k];
        if (cin[k] == 8)
            vt_conv<8, true>(st, VT_IN_BUFFER, dz, idx, np, B, Hk[k], Wk[k], cout[k], w, nullptr, da);
        else
            vt_conv<16, true>(st, VT_IN_BUFFER, dz, idx, np, B, Hk[k], Wk[k], cout[k], w, nullptr, da);
        if (k == 2) {       // da holds the pooled map's gradient: spread it over block 2's output
            hipLaunchKernelGGL(vt_pool_bwd, dim3(vt_blocks((size_t)B * L.P * 8)), block, 0, st, da, sc + S.a[1], B, m, n, other);
            float *swap = da;
            da = other, other = swap;
        }
    }
    WB_HIP_CHECK(hipGetLastError());

    // ---- update
    VtSegments seg;
    for (int s = 0; s < 29; ++s) seg.off[s] = L.off[s];
    VtAdam ad;
    ad.lr = hy.lr, ad.beta1 = hy.beta1, ad.beta2 = hy.beta2;
    ad.b1 = (float)hy.beta1, ad.b2 = (float)hy.beta2, ad.epsilon = (float)hy.adam_epsilon, ad.momentum = (float)hy.momentum;
    hipLaunchKernelGGL(vt_update_kernel, dim3(vt_blocks((size_t)L.off[28])), block, 0, st, params, adam_m, adam_v, t, grad, grads_out,
                       seg, ad);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
