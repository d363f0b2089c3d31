// Box regression: a linear map from a window's channel values to four box offsets, fitted by streaming normal equations
// on the device and applied to detections where their windows lie in the pyramid (the reference computes the target,
// samples.py:152-157, and never uses it).  DESIGN.md 4.15 has the rule, tests/regress_reference.py states it in NumPy,
// tests/regress_designs.py proves designed answers.
//
// wb_gram_launch: S += A^T A, A = [X | 1 | T], N x P, P = D + 5, in float64.
//   gram_partial_kernel  one workgroup per (pair of 64-column panels TI <= TJ, chunk of WB_GRAM_CHUNK rows); wave w owns the
//                        16 output rows 16 w .. 16 w + 15 of the 64 x 64 block and four 16 x 16 tiles across it, each one
//                        accumulator of v_mfma_f64_16x16x4_f64.  Both operands are column panels of the same A: lane l
//                        reads A[k0 + (l >> 4)][i0 + (l & 15)], 16 consecutive features of one row, straight from L2
//                        (the matrix is a few hundred KB), widened exactly.  Rows past n_rows and columns past P read as
//                        zeros, so a short last chunk and N % 4 need no code of their own.  Only tiles ti <= tj are
//                        computed.  The f64 MFMA's C/D map is col = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32
//                        forms' map.  Every computed tile goes to scratch whole: its content on entry does not matter.
//   gram_reduce_kernel   one workgroup per panel pair: an entry i <= j adds its partials in ascending chunk order, adds
//                        that sum to S[i][j], and writes the same bits to S[j][i].
// No floating-point atomics: the result depends on the inputs and the sequence of calls alone, not on the grid or the run.
//
// wb_regress_predict_launch / wb_regress_apply_launch: one wave per window, one body over two loaders (a crop; a window
// where it lies in the pyramid).  Lane l keeps four float64 partials and adds x[j] * W[j][k] for j = l, l + 64, ...
// ascending, product and sum rounded separately (-ffp-contract=off); then p[l] = p[l] + p[l ^ s] for s = 32 .. 1;
// pred[k] = p[0][k] + b[k].  The apply form turns that into the refined box float32(float64(box) - pred * inv64[level]).
#include "wb_match_iou.h"   // window_box: Model.get_boxes' arithmetic; WB_LABEL_MAX_DET

namespace {

typedef double gram_f64x4 __attribute__((ext_vector_type(4)));

constexpr int GRAM_PANEL = 64;                             // columns of a panel: four 16-column MFMA tiles
constexpr int GRAM_BLOCK = GRAM_PANEL * GRAM_PANEL;        // doubles of one (panel pair, chunk) partial

// A[row][col] of [X | 1 | T], zeros outside N x P
template <typename E>
__device__ inline double gram_elem(const E *X, const double *T, int64_t n_rows, int D, int64_t row, int col) {
    if (row >= n_rows) return 0.0;
    if (col < D) return (double)X[row * D + col];
    if (col == D) return 1.0;
    if (col < D + 5) return T[row * 4 + (col - D - 1)];
    return 0.0;
}

// pair index -> (TI, TJ), TI <= TJ < nT, row by row of the upper triangle
__device__ inline void gram_pair(int pair, int nT, int &TI, int &TJ) {
    int ti = 0;
    while (pair >= nT - ti) pair -= nT - ti, ++ti;
    TI = ti, TJ = ti + pair;
}

template <typename E>
__global__ __launch_bounds__(256) void gram_partial_kernel(const E *X, const double *T, int64_t n_rows, int D, int nT, int pairs,
                                                           double *part) {
    const int pair = (int)(blockIdx.x % (uint32_t)pairs);
    const int64_t chunk = blockIdx.x / (uint32_t)pairs;
    int TI, TJ;
    gram_pair(pair, nT, TI, TJ);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, P = D + 5;
    const int ti = TI * 4 + w;                             // this wave's 16 output rows: features 16 ti ..
    if (16 * ti >= P) return;                              // (wave-uniform: nothing of it is read back)
    const int ci = 16 * ti + (lane & 15), cj = TJ * GRAM_PANEL + (lane & 15);
    bool on[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) on[q] = TJ * 4 + q >= ti && 16 * (TJ * 4 + q) < P;
    gram_f64x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = gram_f64x4{0.0, 0.0, 0.0, 0.0};
    const int64_t r0 = chunk * WB_GRAM_CHUNK + (lane >> 4);
    for (int k = 0; k < WB_GRAM_CHUNK; k += 4) {
        const int64_t row = r0 + k;
        const double a = gram_elem(X, T, n_rows, D, row, ci);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!on[q]) continue;                          // (wave-uniform)
            const double b = gram_elem(X, T, n_rows, D, row, cj + 16 * q);
            acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
        }
    }
    double *dst = part + ((size_t)chunk * pairs + pair) * GRAM_BLOCK;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!on[q]) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)                  // the f64 map: row = (lane >> 4) + 4 * reg, col = lane & 15
            dst[(16 * w + (lane >> 4) + 4 * reg) * GRAM_PANEL + 16 * q + (lane & 15)] = acc[q][reg];
    }
}

__global__ __launch_bounds__(256) void gram_reduce_kernel(const double *part, int64_t chunks, int nT, int pairs, int P, double *S) {
    const int pair = blockIdx.x;
    int TI, TJ;
    gram_pair(pair, nT, TI, TJ);
    for (int e = threadIdx.x; e < GRAM_BLOCK; e += 256) {
        const int gi = TI * GRAM_PANEL + (e >> 6), gj = TJ * GRAM_PANEL + (e & 63);
        if (gi > gj || gj >= P) continue;
        const double *src = part + (size_t)pair * GRAM_BLOCK + e;
        double s = src[0];
        for (int64_t c = 1; c < chunks; ++c) s = s + src[(size_t)c * pairs * GRAM_BLOCK];
        const double v = S[(size_t)gi * P + gj] + s;
        S[(size_t)gi * P + gj] = v;
        if (gi != gj) S[(size_t)gj * P + gi] = v;
    }
}

struct GramShape {
    int P, nT, pairs;
    int64_t chunks;
    size_t bytes;
};

inline GramShape gram_shape(int64_t n_rows, int D) {
    GramShape g;
    g.P = D + 5;
    g.nT = (g.P + GRAM_PANEL - 1) / GRAM_PANEL;
    g.pairs = g.nT * (g.nT + 1) / 2;
    g.chunks = (n_rows + WB_GRAM_CHUNK - 1) / WB_GRAM_CHUNK;
    g.bytes = (size_t)g.chunks * (size_t)g.pairs * GRAM_BLOCK * sizeof(double);
    return g;
}

inline int gram_sizes_ok(const char *who, int64_t n_rows, int D) {
    WB_REQUIRE(n_rows >= 0 && D >= 1, "%s: n_rows = %lld, D = %d", who, (long long)n_rows, D);
    if (D > WB_GRAM_MAX_P - 5 || n_rows > WB_LABEL_MAX_DET) {
        wb_set_error("%s: %lld rows of %d features (at most %d rows, P = D + 5 <= %d)", who, (long long)n_rows, D, WB_LABEL_MAX_DET,
                     WB_GRAM_MAX_P);
        return WB_ERR_UNSUPPORTED;
    }
    return WB_OK;
}

// ---- the two loaders of the predict body: feature j = (r * n + c) * C + ch of a window, widened exactly
template <typename E>
struct CropLoader {
    const E *x;
    __device__ double at(int j) const { return (double)x[j]; }
};
template <typename E>
struct LevelLoader {
    const E *x;            // the window's first element in its level
    int rowlen;            // n * C contiguous elements per window row
    int64_t pitch;         // v * C elements between two rows of the level
    __device__ double at(int j) const {
        const int i = j / rowlen;
        return (double)x[i * pitch + (j - i * rowlen)];
    }
};

template <typename L>
__device__ inline void regress_window(const L &ld, int D, const double *Wb, int lane, double pred[4]) {
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < D; j += 64) {
        const double x = ld.at(j);
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = p[k] + x * Wb[4 * (size_t)j + k];
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = p[k] + __shfl_xor(p[k], s, WB_WAVE);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) pred[k] = p[k] + Wb[4 * (size_t)D + k];
}

template <typename E>
__global__ __launch_bounds__(256) void regress_predict_kernel(const E *X, int64_t n, int D, const double *Wb, double *pred) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                    // (wave-uniform)
    const int lane = threadIdx.x & 63;
    double out[4];
    regress_window(CropLoader<E>{X + (size_t)i * D}, D, Wb, lane, out);
    if (lane < 4) pred[4 * i + lane] = lane == 0 ? out[0] : lane == 1 ? out[1] : lane == 2 ? out[2] : out[3];
}

template <typename E>
__global__ __launch_bounds__(256) void regress_apply_kernel(const E *buf, int64_t img_stride, int n_images, const WbMineLevel *levels,
                                                            int n_levels, int C, const WbDet *det, int64_t n_det, int m, int n,
                                                            const double *Wb, const float *inv_scale, const double *inv64, double *pred,
                                                            float *boxes, uint32_t *err) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_det) return;                                // (wave-uniform, as everything below that depends on the record alone)
    const int lane = threadIdx.x & 63;
    const WbDet d = det[i];
    bool ok = d.image >= 0 && d.image < n_images && d.level >= 0 && d.level < n_levels;
    const int level = d.level < 0 ? 0 : (d.level >= n_levels ? n_levels - 1 : d.level);
    int64_t base = 0, pitch = 0;
    if (ok) {                                              // wb_mine_gather_launch's test, before anything is read
        const WbMineLevel lv = levels[d.level];
        ok = lv.u >= 0 && lv.v >= 0 && (int)d.r + m <= lv.u && (int)d.c + n <= lv.v && lv.chn_off >= 0 &&
             lv.chn_off + (int64_t)lv.u * lv.v * C <= img_stride;
        pitch = (int64_t)lv.v * C;
        base = (int64_t)d.image * img_stride + lv.chn_off + ((int64_t)d.r * lv.v + d.c) * C;
    }
    const float4 box = window_box(inv_scale[level], d.r, d.c, m, n);
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) regress_window(LevelLoader<E>{buf + base, n * C, pitch}, m * n * C, Wb, lane, out);
    if (lane >= 4) return;
    const double p = lane == 0 ? out[0] : lane == 1 ? out[1] : lane == 2 ? out[2] : out[3];
    const float b = lane == 0 ? box.x : lane == 1 ? box.y : lane == 2 ? box.z : box.w;
    if (pred) pred[4 * i + lane] = p;
    boxes[4 * i + lane] = ok ? (float)((double)b - p * inv64[level]) : b;
    if (!ok && lane == 0) atomicOr(err, 1u);
}

inline int regress_window_ok(const char *who, int64_t count, int m, int n, int C, int dtype) {
    WB_REQUIRE(count >= 0, "%s: negative count", who);
    WB_REQUIRE(m >= 1 && n >= 1 && C >= 1 && (int64_t)m * n * C < (1ll << 24), "%s: window %d x %d x %d", who, m, n, C);
    if (dtype != WB_DTYPE_F32 && dtype != WB_DTYPE_U8) {
        wb_set_error("%s: dtype %d (float32 and uint8 channels have windows)", who, dtype);
        return WB_ERR_UNSUPPORTED;
    }
    if (count > WB_LABEL_MAX_DET) {
        wb_set_error("%s: %lld windows (at most %d in one call)", who, (long long)count, WB_LABEL_MAX_DET);
        return WB_ERR_UNSUPPORTED;
    }
    return WB_OK;
}

}  // namespace

extern "C" int wb_gram_scratch_bytes(int64_t n_rows, int D, size_t *bytes) {
    WB_REQUIRE(bytes, "wb_gram_scratch_bytes: null pointer");
    const int rc = gram_sizes_ok("wb_gram_scratch_bytes", n_rows, D);
    if (rc != WB_OK) return rc;
    *bytes = gram_shape(n_rows, D).bytes;
    return WB_OK;
}

extern "C" int wb_gram_launch(void *stream, const void *X, int x_dtype, const double *T, int64_t n_rows, int D, double *S, void *scratch,
                              size_t scratch_bytes) {
    const int rc = gram_sizes_ok("wb_gram_launch", n_rows, D);
    if (rc != WB_OK) return rc;
    if (x_dtype != WB_DTYPE_F32 && x_dtype != WB_DTYPE_U8) {
        wb_set_error("wb_gram_launch: x_dtype %d (float32 and uint8 features)", x_dtype);
        return WB_ERR_UNSUPPORTED;
    }
    if (n_rows == 0) return WB_OK;
    WB_REQUIRE(X && T && S && scratch, "wb_gram_launch: null pointer");
    WB_REQUIRE(wb_aligned(T, 8) && wb_aligned(S, 8) && wb_aligned(scratch, 8) && (x_dtype == WB_DTYPE_U8 || wb_aligned(X, 4)),
               "wb_gram_launch: T, S and scratch must be 8-byte aligned, float32 X 4-byte aligned");
    const GramShape g = gram_shape(n_rows, D);
    WB_REQUIRE(scratch_bytes >= g.bytes, "wb_gram_launch: scratch of %zu bytes, %zu needed", scratch_bytes, g.bytes);
    WB_REQUIRE(g.chunks * g.pairs < (1ll << 31), "wb_gram_launch: %lld chunks of %d panel pairs in one call", (long long)g.chunks, g.pairs);
    hipStream_t st = (hipStream_t)stream;
    double *part = static_cast<double *>(scratch);
    const dim3 grid((uint32_t)(g.chunks * g.pairs)), wg(256);
    if (x_dtype == WB_DTYPE_F32)
        hipLaunchKernelGGL((gram_partial_kernel<float>), grid, wg, 0, st, static_cast<const float *>(X), T, n_rows, D, g.nT, g.pairs, part);
    else
        hipLaunchKernelGGL((gram_partial_kernel<uint8_t>), grid, wg, 0, st, static_cast<const uint8_t *>(X), T, n_rows, D, g.nT, g.pairs, part);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((uint32_t)g.pairs), wg, 0, st, part, g.chunks, g.nT, g.pairs, g.P, S);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_regress_predict_launch(void *stream, const void *X, int x_dtype, int64_t n, int m, int nn, int C, const double *Wb,
                                         double *pred) {
    const int rc = regress_window_ok("wb_regress_predict_launch", n, m, nn, C, x_dtype);
    if (rc != WB_OK) return rc;
    if (n == 0) return WB_OK;
    WB_REQUIRE(X && Wb && pred, "wb_regress_predict_launch: null pointer");
    WB_REQUIRE(wb_aligned(Wb, 8) && wb_aligned(pred, 8) && (x_dtype == WB_DTYPE_U8 || wb_aligned(X, 4)),
               "wb_regress_predict_launch: Wb and pred must be 8-byte aligned, float32 X 4-byte aligned");
    const dim3 grid((uint32_t)((n + 3) / 4)), wg(256);
    hipStream_t st = (hipStream_t)stream;
    const int D = m * nn * C;
    if (x_dtype == WB_DTYPE_F32)
        hipLaunchKernelGGL((regress_predict_kernel<float>), grid, wg, 0, st, static_cast<const float *>(X), n, D, Wb, pred);
    else
        hipLaunchKernelGGL((regress_predict_kernel<uint8_t>), grid, wg, 0, st, static_cast<const uint8_t *>(X), n, D, Wb, pred);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_regress_apply_launch(void *stream, const void *buf, int dtype, int64_t img_stride, int n_images, const WbMineLevel *levels,
                                       int n_levels, int C, const WbDet *det, int64_t n_det, int m, int nn, const double *Wb,
                                       const float *inv_scale, const double *inv64, double *pred, float *boxes, uint32_t *err) {
    const int rc = regress_window_ok("wb_regress_apply_launch", n_det, m, nn, C, dtype);
    if (rc != WB_OK) return rc;
    WB_REQUIRE(img_stride >= 0 && n_images >= 0 && n_levels >= 0, "wb_regress_apply_launch: img_stride = %lld, n_images = %d, n_levels = %d: negative",
               (long long)img_stride, n_images, n_levels);
    WB_REQUIRE(err, "wb_regress_apply_launch: null pointer");
    WB_REQUIRE(wb_aligned(err, 4), "wb_regress_apply_launch: err must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n_det == 0) {
        WB_HIP_CHECK(hipMemsetAsync(err, 0, 4, st));
        return WB_OK;
    }
    WB_REQUIRE(buf && levels && det && Wb && inv_scale && inv64 && boxes, "wb_regress_apply_launch: null pointer");
    WB_REQUIRE(n_levels >= 1, "wb_regress_apply_launch: %lld records of no level", (long long)n_det);
    WB_REQUIRE(wb_aligned(det, 16) && wb_aligned(levels, 8) && wb_aligned(Wb, 8) && wb_aligned(inv64, 8) && wb_aligned(pred, 8) &&
                   wb_aligned(inv_scale, 4) && wb_aligned(boxes, 4) && (dtype == WB_DTYPE_U8 || wb_aligned(buf, 4)),
               "wb_regress_apply_launch: det 16-byte, levels, Wb, inv64 and pred 8-byte, inv_scale, boxes and float buffers 4-byte aligned");
    WB_HIP_CHECK(hipMemsetAsync(err, 0, 4, st));
    const dim3 grid((uint32_t)((n_det + 3) / 4)), wg(256);
    if (dtype == WB_DTYPE_F32)
        hipLaunchKernelGGL((regress_apply_kernel<float>), grid, wg, 0, st, static_cast<const float *>(buf), img_stride, n_images, levels, n_levels,
                           C, det, n_det, m, nn, Wb, inv_scale, inv64, pred, boxes, err);
    else
        hipLaunchKernelGGL((regress_apply_kernel<uint8_t>), grid, wg, 0, st, static_cast<const uint8_t *>(buf), img_stride, n_images, levels,
                           n_levels, C, det, n_det, m, nn, Wb, inv_scale, inv64, pred, boxes, err);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
