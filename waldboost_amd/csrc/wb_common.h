// Internal helpers shared by the gfx950 kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/waldboost_hip.h"
#include "wb_stage_records.h"   // tile forms, cascade geometry constants, the stage record, host canonicalisation

#define WB_WAVE 64

// ---- error plumbing: wb_set_error and WB_REQUIRE are in wb_stage_records.h (no HIP in them) ----
#define WB_HIP_CHECK(expr)                                                             \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            wb_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return WB_ERR_HIP;                                                         \
        }                                                                              \
    } while (0)

// ---- order-preserving uint32 keys for min/max atomics ----
// uint8 pixels use their value; float32 uses the usual sign-flip encoding so that
// unsigned comparison of keys == float comparison of values.
__host__ __device__ inline uint32_t wb_f32_key(float f) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float wb_key_f32(uint32_t k) {
    uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

// the smallest key of a wave, in every lane
__device__ inline uint32_t wb_wave_min_u32(uint32_t k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)k, off, WB_WAVE);
        k = o < k ? o : k;
    }
    return k;
}
// T keys of minima back to floats, in place, behind the work on the stream (wb_cascade.hip); all ones -- a minimum over
// nothing -- becomes +inf
int wb_keys_to_floats_launch(hipStream_t st, uint32_t *keys, int T);

// ---- a launcher's alignment test (host)
inline bool wb_aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// ---- how a float64-held image dtype is cast back after the resize / pooled in the octaves (WB_DTYPE_F64 .. WB_DTYPE_F16) ----
#define WB_CAST_NONE 0     // float64
#define WB_CAST_TRUNC 1    // integers: truncation toward zero
#define WB_CAST_BOOL 2     // bool: != 0
#define WB_CAST_F16 3      // float16: round to nearest even
inline int wb_cast_mode(int dtype) {
    switch (dtype) {
        case WB_DTYPE_F64: return WB_CAST_NONE;
        case WB_DTYPE_BOOL: return WB_CAST_BOOL;
        case WB_DTYPE_F16: return WB_CAST_F16;
        default: return WB_CAST_TRUNC;
    }
}
inline bool wb_dtype_held_f64(int dtype) { return dtype == WB_DTYPE_F64 || (dtype >= WB_DTYPE_I8 && dtype <= WB_DTYPE_F16); }
// a double rounded to binary16 (round to nearest even, one rounding): to float32 toward zero with the sticky bit kept
// in the last place (round to odd), then the hardware's float32 -> float16 conversion
__device__ inline double wb_round_f16(double x) {
    float f = __double2float_rz(x);
    if ((double)f != x) f = __uint_as_float(__float_as_uint(f) | 1u);     // (inexact; a NaN stays a NaN)
    return (double)(float)(_Float16)f;
}

// One tile form of a model (WbTileForm): its stage records and the tile kernel's needs for them
struct WbFormRecords {
    int present;            // 1 = the model can be scanned in this form (the rank forms: its thresholds fit the tables)
    int owned;              // 1 = the two stage tables are this handle's to free (0: a member view sharing its model's)
    int32_t *stages_dev;    // (n_stages + G) stage records
    int32_t *stages_host;   // the byte forms: host copy the generator of the specialised kernel bakes in
    int lds_bytes;          // dynamic LDS of the tile kernel
    int rpw;                // window rows per wave of this form's tile kernel (the model's, or twice that: choose_geometry)
    int tile_rows;          // = rpw * waves: a multiple of the model's tile_rows, the unit of the tile table
    int lds_rows;           // tile_rows + m - 1
    int elem_bytes;         // wb_form_elem_bytes
    void *jit;              // model-specialised kernel (wb_jit.hip, wb_model_specialize): hipFunction_t, or null; always the handle's own
    int refused;            // 1 = its specialised kernel failed the self-test, no retry
};

// Threshold ranks of float32 channel values (written by the channel kernel, scanned by the byte-tile cascade kernels): per
// channel the model's distinct thresholds are sorted, a pixel is replaced by the number of them below it (its rank), and a
// node test `v <= thr` becomes `rank(v) <= index(thr)` -- the same decision for every float, in a quarter or half of the bytes
struct WbRankTable {
    int iters;              // K: most thresholds that share one cell of the lookup grid (refinement steps per pixel)
    float k[4], b[4];       // cell(v) = trunc(clamp(fma(v, k[c], b[c]), 0, cells - 1))
    uint8_t *lut_dev;       // float S[4][slots] (sorted thresholds, +inf padded), then base[4][cells]: WB_BIN_* / WB_BIN16_*
    int owned;              // 1 = lut_dev is this handle's to free (0: a member view: the group's)
};

struct WbModel {
    int n_stages, depth, m, n, C;
    int rpw;          // window rows per wave in the cascade tile: the float32 form's, and the least of any form
    int waves;        // wavefronts per workgroup
    int tile_rows;    // = rpw * waves: the unit of WbTile.ty (a form's own tile is this tall or a multiple: WbFormRecords)
    int lds_rows;     // tile_rows + m - 1
    int lds_pitch;    // WB_CASC_TC + n - 1 pixels + 1 pad column
    int lds_stages;   // stage records mirrored in LDS (n_stages if the table is <= 16 KiB, else 0)
    int stage_dwords;
    size_t stage_words;                   // (n_stages + G) * stage_dwords: words of every form's stage table
    WbFormRecords form[WB_FORM_COUNT];    // none present on a generic model
    WbRankTable ranks[2];                 // of WB_FORM_RANK8 and WB_FORM_RANK16 (wb_rank_table)
    int jit_off;                // 1 = wb_cascade_launch ignores the loaded specialised kernels (wb_model_use_specialized)
    int proxy;                  // 1 = a member view of a WbRankGroup: everything below is its model's
    // host copy of the caller's tree arrays (wb_rankgroup_create derives stage records for a shared rank table from them)
    int n_nodes;
    int32_t *h_node_off;        // [n_stages + 1]
    uint8_t *h_feature;         // [n_nodes][3]
    float *h_threshold, *h_prediction, *h_theta;
    int8_t *h_left, *h_right;
    // trees deeper than WB_CASC_MAX_DEPTH: generic node-walk kernel on the reference's own flat arrays
    int generic;                // 1 = use cascade_generic_kernel
    int32_t *g_node_off;        // [n_stages + 1]
    int32_t *g_feat;            // [n_nodes] row | col << 8 | channel << 16
    float *g_thr;               // [n_nodes]
    int32_t *g_left, *g_right;  // [n_nodes] child index inside the stage's tree, -1 on leaves
    float *g_pred;              // [n_nodes]
    float *g_theta;             // [n_stages]
};
inline const WbRankTable &wb_rank_table(const WbModel *model, int form) { return model->ranks[form - WB_FORM_RANK8]; }

// ---- the tile kernel's host side (wb_cascade.hip), as wb_model_create needs it ----
#ifndef WB_CASC_BYTE_RPW
#define WB_CASC_BYTE_RPW 8      // rows per wave of the one-byte forms' tile (choose_geometry): 64 x 64 windows on eight waves
#endif
bool wb_cascade_has_kernel(int depth, int rpw, int waves);   // an instance of the tile kernel exists for this shape
int wb_cascade_prepare(int depth, int rpw, int waves);  // the instances' dynamic-LDS limit raised; WB_ERR_UNSUPPORTED: no kernel for this shape
int wb_cascade_group(int depth);                        // stages evaluated per group
int wb_cascade_lds_bytes(int eb, int C, int rows, int pitch, int TR, int waves, int T, int lds_stages,
                         int depth);                    // dynamic LDS of the tile kernel

// ---- model-specialised kernels (wb_jit.hip), as wb_model_specialize needs them ----
int wb_jit_get(const int32_t *words, size_t n_words, int T, int D, int rpw, int waves, int C, int rows, int pitch, int eb,
               int lds_stages, void **func_out);
void wb_jit_release(void *func);
int wb_jit_selftest(WbModel *model, int chn_dtype, WbFormRecords *rec);   // WB_ERR_UNSUPPORTED: rec->jit disagreed with the generic kernel

// ---- threshold ranks of float32 channel values (WbRankTable, WB_DTYPE_RANK8) ----
// cell of a channel's lookup grid (host mirror: bin_cell() in wb_stage_records.h): non-decreasing in v
__device__ inline uint32_t wb_bin_cell(float v, float k, float b, float top = (float)(WB_BIN_CELLS - 1)) {
    const float q = __builtin_amdgcn_fmed3f(__builtin_fmaf(v, k, b), 0.0f, top);
    return (uint32_t)q;
}
// rank of v among the channel's sorted distinct thresholds S (+inf padded): the number of them below v.
// base[cell] counts the thresholds of lower cells (all below v); the thresholds of v's own cell follow in S, in
// order, at most K of them; thresholds of higher cells are above v.  (NaN: the caller substitutes 255.)
__device__ inline uint32_t wb_bin_rank(float v, float k, float b, const uint8_t *base, const float *S, int K) {
    uint32_t r = base[wb_bin_cell(v, k, b)];
    for (int i = 0; i < K; ++i) r += v > S[r] ? 1u : 0u;
    return r;
}
