// Evaluation of the WaldBoost decision trees on gfx950: everything that walks a tree.
//
// Replaces reference model.py:216-259 (Model.predict_on_image: window grid, stage loop,
// rejection, compaction, n_loc/n_weak statistics) and training.py:84-96
// (DTree.predict_on_image: the tree walk on all alive windows).
//
// This file holds
//   * cascade_tile_kernel<D, RPW, WAVES, EB>: the instances of the tiled cascade (body in wb_cascade_tile.h, design below),
//     casc_dispatch from a model's run-time (depth, rows per wave, waves) to them, wb_cascade_prepare and
//     wb_cascade_launch / wb_cascade_launch_z;
//   * cascade_generic_kernel: the node-walk fallback for models without a tile kernel;
//   * training-time callers of the same walks: tree_eval_kernel (wb_tree_eval_launch), samples_predict_kernel
//     (wb_samples_predict_launch), tree_apply_kernel (wb_tree_apply_launch) and gather_samples_kernel
//     (wb_gather_samples_launch);
//   * threshold calibration on samples: samples_trace_kernel (wb_samples_trace_launch: the running score after every
//     stage, per-stage survival) and calib_min_kernel (wb_calib_min_launch: per-stage minimum over the retained samples).
// The two walks -- a stage of the model's flat arrays, one tree's uint8 / int8 arrays -- stand here once each (flat_stage,
// tree_leaf).  What reads the detection records the cascade leaves is in wb_det.hip.
//
// The tiled cascade: one workgroup owns a tile of TR x 64 windows of one level of one image (TR per tile form: 32 rows,
// 64 on the one-byte forms where 40 KB of LDS hold them -- wb_model.hip, choose_geometry):
//   * the (TR+m-1) x (64+n-1) x C channel block is staged once into LDS, planar, so that a
//     wavefront's 64 lanes (64 adjacent window columns) gather from 64 adjacent banks;
//   * wave-synchronous stages: every lane of a wave is at the same stage, so the stage records
//     come in through the scalar cache (s_load) and cost no vector memory or LDS traffic; stages
//     are evaluated in groups of G with all 2*G gathers in flight (only the fp32 accumulation
//     and the rejection tests are sequential);
//   * phase A runs the first stages with RPW windows per lane, four rows at a time; survivors are compacted with
//     wave ballot + mbcnt into the wave's own LDS queue; phase B re-packs them densely for
//     geometrically growing stage segments, compacting in place after each segment, and pools
//     the survivors of the whole workgroup once, at stage 8, so that a few waves hold full
//     chunks of 64 and the rest retire;
//   * stage-parallel tail: once a wave is down to a handful of windows (about 1e-3 of the
//     windows of the benchmark cascade reach stage 32, with ~100 stages to go) the roles flip:
//     four windows at a time, 16 stages of each AT ONCE, one stage per lane (per-lane stage records,
//     gathers from the same LDS tile); the fp32 accumulation and the rejection tests are then
//     replayed in stage order (a DPP row_shr:1 ripple inside each 16-lane row: lane i of a row ends up
//     with ((h+p_0)+p_1)+...+p_i, exactly the reference's running sum) -- so a nearly empty wave no
//     longer walks 100 stages serially while the workgroup's LDS tile sits idle;
//   * the windows alive after the last dense stage stay in the wave's queue and every wave that holds
//     some reserves their output slots with ONE atomic on one of WB_DET_SHARDS counters; a window that
//     passes the last stage in the tail is appended right there.
//
// Scores are accumulated in fp32 strictly in stage order and compared with `>=`, so they are
// bit-identical to the reference's `hs += ...; mask = hs >= theta`.
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "wb_common.h"

#include "wb_cascade_tile.h"

namespace {

template <int D, int RPW, int WAVES, int EB>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_num_sgpr(80))) void cascade_tile_kernel(CascArgs a, const int32_t *__restrict__ stages) {
    cascade_tile_body<D, RPW, WAVES, EB, false>(a, stages);
}

// -------------------------------------------------------------------------------------------
// The two tree walks of the reference (training.py:84-96), on whatever pixels the caller's fetch gives.

// a channel value: element `at` of float32 or uint8 channels
__device__ inline float chn_at(const void *X, int x_u8, int64_t at) {
    return x_u8 ? (float)reinterpret_cast<const uint8_t *>(X)[at] : reinterpret_cast<const float *>(X)[at];
}

// the model's flat node arrays: the trees of all stages back to back (stage t: nodes node_off[t] .. node_off[t + 1])
struct FlatModel {
    int T, m, n, C;
    const int32_t *node_off, *feat, *left, *right;     // feat: row | col << 8 | channel << 16; children inside the stage's tree, -1 on leaves
    const float *thr, *pred, *theta;
};
FlatModel flat_model(const WbModel *model) {
    return {model->n_stages, model->m, model->n, model->C, model->g_node_off, model->g_feat, model->g_left, model->g_right,
            model->g_thr, model->g_pred, model->g_theta};
}

// stage t on the window whose pixel (row, col, channel) is fetch(row, col, channel): h += the leaf's prediction, in
// fp32; false = rejected (the reference's `hs += ...; mask = hs >= theta`, theta = -inf never rejects)
template <typename Fetch>
__device__ inline bool flat_stage(const FlatModel &a, int t, float &h, Fetch &&fetch) {
    const int o = a.node_off[t], k = a.node_off[t + 1] - o;
    int node = 0;
    for (int step = 0; step < k; ++step) {                            // a walk visits a node at most once
        const int l = a.left[o + node];
        if (l < 0) break;
        const int f = a.feat[o + node];
        node = (fetch(f & 255, (f >> 8) & 255, (f >> 16) & 255) <= a.thr[o + node]) ? l : a.right[o + node];
    }
    h = h + a.pred[o + node];
    const float th = a.theta[t];
    return (th == -INFINITY) || (h >= th);
}

// one tree as DTree holds it (uint8 feature[n_nodes][3], int8 children): the leaf the window lands in
template <typename Fetch>
__device__ inline int tree_leaf(const uint8_t *feature, const float *threshold, const int8_t *left, const int8_t *right,
                                int n_nodes, Fetch &&fetch) {
    int node = 0;
    for (int step = 0; step < n_nodes; ++step) {          // bounded: a walk visits each node at most once
        const int l = left[node];
        if (l < 0) break;
        node = (fetch(feature[node * 3 + 0], feature[node * 3 + 1], feature[node * 3 + 2]) <= threshold[node]) ? l : (int)right[node];
    }
    return node;
}

// -------------------------------------------------------------------------------------------
// Generic fallback for trees deeper than WB_CASC_MAX_DEPTH (or any shape): one thread per window,
// 4 x 64 windows per workgroup, the reference's flat node arrays walked as training.py:84-96 does,
// features gathered straight from HBM/L2.  Wave-synchronous in the stage index (dead lanes idle),
// so the per-stage alive counts are ballots; survivors leave through an LDS list and one sharded
// atomic per workgroup, like the tiled kernel.  Correctness fallback, not a tuned path.
struct GenArgs {
    FlatModel model;
    const void *chn;
    int chn_u8;
    int64_t chn_stride;
    const WbLevel *levels;
    const WbTile *tiles;
    int n_levels, n_tiles;
    WbDet *det;
    uint32_t *det_count;
    uint32_t det_cap;
    uint32_t *alive;
    uint32_t *zero;
    int zero_words;
};

__global__ __launch_bounds__(256) void cascade_generic_kernel(GenArgs a) {
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < a.zero_words; i += 256) a.zero[i] = 0u;      // (see cascade_tile_body)
    const int T = a.model.T;
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(gsm);                       // T counters
    uint2 *list = reinterpret_cast<uint2 *>(gsm + (((size_t)T * 4 + 15) & ~(size_t)15));   // 256 entries
    __shared__ uint32_t n_list, base_slot;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const WbTile tile_d = a.tiles[blockIdx.x];
    const WbLevel L = a.levels[tile_d.level];
    const int b = blockIdx.y;
    const int nr = L.u - a.model.m > 0 ? L.u - a.model.m : 0, nc = L.v - a.model.n > 0 ? L.v - a.model.n : 0;
    const int r = tile_d.ty * 4 + wave, c = tile_d.tx * 64 + lane;
    for (int t = tid; t < T; t += 256) hist[t] = 0;
    if (tid == 0) n_list = 0;
    __syncthreads();
    const int64_t level0 = (int64_t)b * a.chn_stride + L.chn_off;             // the level's first element
    bool alive = r < nr && c < nc;
    float h = 0.f;
    for (int t = 0; t < T; ++t) {
        int cnt = __popcll(__ballot(alive));
        if (cnt == 0) break;
        if (lane == 0) atomicAdd(&hist[t], (uint32_t)cnt);
        if (alive)
            alive = flat_stage(a.model, t, h, [&](int fr, int fc, int ch) {
                return chn_at(a.chn, a.chn_u8, level0 + ((int64_t)(r + fr) * L.v + (c + fc)) * a.model.C + ch);
            });
    }
    if (alive) {
        uint32_t s = atomicAdd(&n_list, 1u);
        list[s] = make_uint2((uint32_t)(wave * 64 + lane), __float_as_uint(h));
    }
    __syncthreads();
    const uint32_t shard = blockIdx.x % WB_DET_SHARDS;
    if (tid == 0) base_slot = n_list ? atomicAdd(a.det_count + shard, n_list) : 0u;
    if (a.alive) {
        uint32_t *al = a.alive + ((int64_t)b * a.n_levels + tile_d.level) * T;
        for (int t = tid; t < T; t += 256)
            if (hist[t]) atomicAdd(al + t, hist[t]);
    }
    __syncthreads();
    if ((uint32_t)tid < n_list) {
        uint2 e = list[tid];
        uint32_t slot = base_slot + tid;
        if (slot < a.det_cap) {
            WbDet d;
            d.image = b;
            d.level = tile_d.level;
            d.r = (uint16_t)(tile_d.ty * 4 + (int)(e.x >> 6));
            d.c = (uint16_t)(tile_d.tx * 64 + (int)(e.x & 63));
            d.score = __uint_as_float(e.y);
            a.det[(size_t)shard * a.det_cap + slot] = d;
        }
    }
}

// -------------------------------------------------------------------------------------------
// DTree.predict_on_image on explicit window lists (reference training.py:84-96)
__global__ void tree_eval_kernel(const void *Xv, int x_u8, int u, int v, int C, const int32_t *rs, const int32_t *cs,
                                 int64_t n_pos, const uint8_t *feature, const float *threshold,
                                 const int8_t *left, const int8_t *right, const float *prediction,
                                 int n_nodes, float *out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pos) return;
    const int r = rs[i], c = cs[i];
    out[i] = prediction[tree_leaf(feature, threshold, left, right, n_nodes, [&](int fr, int fc, int ch) {
        return chn_at(Xv, x_u8, ((int64_t)(r + fr) * v + (c + fc)) * C + ch);
    })];
}

// -------------------------------------------------------------------------------------------
// Training-time callers of the hot path (reference samples.py:14-43, model.py:181-214, training.py:73-83)

// gather_samples: one wave per sample copies its m x n x C crop, row by row (a crop row is n*C
// contiguous elements in X); VEC = elements moved per lane and step
template <typename E>
__global__ __launch_bounds__(64) void gather_samples_kernel(const E *X, int v, int rowlen, const int32_t *rs,
                                                            const int32_t *cs, int m, int xstride, E *out) {
    const int64_t i = blockIdx.x;
    const E *src = X + ((int64_t)rs[i] * v + cs[i]) * xstride;
    E *dst = out + i * (int64_t)m * rowlen;
    const int total = m * rowlen;
    for (int e = threadIdx.x; e < total; e += 64) {
        const int y = e / rowlen, x = e - y * rowlen;
        dst[e] = src[(int64_t)y * v * xstride + x];
    }
}

// Model.predict on samples (m x n x C crops back to back): one thread per sample, the reference's flat node arrays
__global__ __launch_bounds__(256) void samples_predict_kernel(FlatModel a, const void *X, int x_u8, int64_t n_samples, float *H,
                                                              uint8_t *mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_samples) return;
    const int64_t base = i * (int64_t)a.m * a.n * a.C;
    float h = 0.f;
    bool alive = true;
    for (int t = 0; t < a.T && alive; ++t)
        alive = flat_stage(a, t, h, [&](int fr, int fc, int ch) { return chn_at(X, x_u8, base + ((fr * a.n + fc) * a.C + ch)); });
    H[i] = alive ? h : -INFINITY;
    mask[i] = alive ? 1 : 0;
}

// -------------------------------------------------------------------------------------------
// Threshold calibration (direct backward pruning): the running score of a sample after EVERY stage, and the per-stage
// minimum of it over the samples a final-score floor retains.  One thread per sample, 256 samples per workgroup, the same
// walk (flat_stage) as samples_predict_kernel; a wave is at one stage at a time, so the counts are ballots and a stage's
// 64 running scores leave as one 256-byte store.  Per-stage results of a workgroup meet in an LDS table of WB_CALIB_CHUNK
// stages at a time (any number of stages) and reach memory with one atomic per (workgroup, stage).
#define WB_CALIB_CHUNK 1024

// pixel (row, col, channel) of sample i of X[n_samples][m][n][C]
struct SampleFetch {
    const void *X;
    int x_u8, n, C;
    int64_t base;
    __device__ float operator()(int fr, int fc, int ch) const { return chn_at(X, x_u8, base + ((fr * n + fc) * C + ch)); }
};

struct TraceArgs {
    FlatModel model;
    const void *X;
    int x_u8, reject;
    int64_t n_samples;
    float *trace, *fin;      // [T][n_samples], [n_samples]
    uint32_t *alive;         // [T + 1], zeroed ahead of the launch
};

__global__ __launch_bounds__(256) void samples_trace_kernel(TraceArgs a) {
    __shared__ uint32_t hist[WB_CALIB_CHUNK];
    const int T = a.model.T, tid = threadIdx.x, lane = tid & 63;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid, N = a.n_samples;
    const bool valid = i < N;                                  // (no early return: every thread meets the barriers)
    const SampleFetch fetch = {a.X, a.x_u8, a.model.n, a.model.C, (valid ? i : 0) * (int64_t)a.model.m * a.model.n * a.model.C};
    float h = 0.f;
    bool alive = valid;
    // slot t of the counts: samples entering stage t; slot T: those that passed every stage
    for (int t0 = 0; t0 <= T; t0 += WB_CALIB_CHUNK) {
        const int t1 = t0 + WB_CALIB_CHUNK < T + 1 ? t0 + WB_CALIB_CHUNK : T + 1;
        if (a.alive) {
            for (int k = tid; k < t1 - t0; k += 256) hist[k] = 0u;
            __syncthreads();
        }
        for (int t = t0; t < t1; ++t) {
            if (a.alive) {
                const int cnt = __popcll(__ballot(alive));
                if (lane == 0 && cnt) atomicAdd(&hist[t - t0], (uint32_t)cnt);
            }
            if (t == T) break;
            if (alive) {
                const bool pass = flat_stage(a.model, t, h, fetch);
                alive = a.reject ? pass : true;
            }
            if (a.trace && valid) a.trace[(int64_t)t * N + i] = alive ? h : -INFINITY;
        }
        if (a.alive) {
            __syncthreads();
            for (int k = tid; k < t1 - t0; k += 256)          // (the thread that zeroes slot k for the next chunk)
                if (hist[k]) atomicAdd(a.alive + t0 + k, hist[k]);
        }
    }
    if (a.fin && valid) a.fin[i] = alive ? h : -INFINITY;
}

struct CalibArgs {
    FlatModel model;
    const void *X;
    int x_u8;
    float floor;
    int64_t n_samples;
    uint32_t *keys;          // [T] order-preserving keys (wb_f32_key) of the minima, all ones ahead of the launch
    uint32_t *n_retained;    // [1], zeroed ahead of the launch
};

__global__ __launch_bounds__(256) void calib_min_kernel(CalibArgs a) {
    __shared__ uint32_t slot[WB_CALIB_CHUNK];
    __shared__ uint32_t kept;
    const int T = a.model.T, tid = threadIdx.x, lane = tid & 63;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool valid = i < a.n_samples;
    const SampleFetch fetch = {a.X, a.x_u8, a.model.n, a.model.C, (valid ? i : 0) * (int64_t)a.model.m * a.model.n * a.model.C};
    if (tid == 0) kept = 0u;
    // the unrejected final score decides who is retained ...
    float h = 0.f;
    if (valid)
        for (int t = 0; t < T; ++t) flat_stage(a.model, t, h, fetch);
    const bool retained = valid && h >= a.floor;
    const unsigned long long wave_kept = __ballot(retained);
    __syncthreads();
    if (lane == 0 && wave_kept) atomicAdd(&kept, (uint32_t)__popcll(wave_kept));
    // ... and the same walk again gives the retained samples' running scores, stage by stage (no trace is stored): the key
    // in a register, the wave's smallest, the workgroup's in LDS, one atomic min per stage
    h = 0.f;
    for (int t0 = 0; t0 < T; t0 += WB_CALIB_CHUNK) {
        const int t1 = t0 + WB_CALIB_CHUNK < T ? t0 + WB_CALIB_CHUNK : T;
        for (int k = tid; k < t1 - t0; k += 256) slot[k] = 0xFFFFFFFFu;
        __syncthreads();
        if (wave_kept)
            for (int t = t0; t < t1; ++t) {
                if (retained) flat_stage(a.model, t, h, fetch);
                const uint32_t k = wb_wave_min_u32(retained ? wb_f32_key(h) : 0xFFFFFFFFu);
                if (lane == 0) atomicMin(&slot[t - t0], k);
            }
        __syncthreads();
        for (int k = tid; k < t1 - t0; k += 256)              // (the thread that resets slot k for the next chunk)
            if (slot[k] != 0xFFFFFFFFu) atomicMin(a.keys + t0 + k, slot[k]);
    }
    __syncthreads();
    if (tid == 0 && kept) atomicAdd(a.n_retained, kept);
}

// keys of minima back to floats, in place; all ones (no sample reached the stage, no bag) becomes +inf: wb_keys_to_floats_launch
__global__ __launch_bounds__(256) void calib_keys_kernel(uint32_t *keys, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const uint32_t k = keys[t];
    reinterpret_cast<float *>(keys)[t] = k == 0xFFFFFFFFu ? INFINITY : wb_key_f32(k);
}

// DTree.apply on samples
__global__ __launch_bounds__(256) void tree_apply_kernel(const void *Xv, int x_u8, int64_t n_samples, int m, int n, int C,
                                                         const uint8_t *feature, const float *threshold,
                                                         const int8_t *left, const int8_t *right, int n_nodes,
                                                         int32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_samples) return;
    const int64_t base = i * (int64_t)m * n * C;
    out[i] = tree_leaf(feature, threshold, left, right, n_nodes,
                       [&](int fr, int fc, int ch) { return chn_at(Xv, x_u8, base + ((fr * n + fc) * C + ch)); });
}

// -------------------------------------------------------------------------------------------
// The tile kernel's instances: rows per wave x waves, for depths 1 .. WB_CASC_MAX_DEPTH and the three tile element forms
// (EB: 0 float32, 1 bytes, 2 16-bit ranks)
#define WB_CASC_CONFIGS(X) X(8, 4) X(4, 4) X(2, 4) X(1, 4) X(8, 8) X(4, 8) X(2, 8) X(1, 8) X(2, 16) X(1, 16)

// run-time (depth, rpw, waves) -> compile-time constants: f(integral_constant D, RPW, WAVES), whose int result is handed
// back; the one error for a shape without kernels.  wb_model_create refuses such a model (wb_cascade_prepare), so a
// launch never meets it.
template <int V> using Int = std::integral_constant<int, V>;
template <typename F> int casc_dispatch(int depth, int rpw, int waves, F &&f) {
#define WB_X(R, W)                                          \
    if (rpw == R && waves == W) switch (depth) {            \
            case 1: return f(Int<1>{}, Int<R>{}, Int<W>{}); \
            case 2: return f(Int<2>{}, Int<R>{}, Int<W>{}); \
            case 3: return f(Int<3>{}, Int<R>{}, Int<W>{}); \
        }
    WB_CASC_CONFIGS(WB_X)
#undef WB_X
    static_assert(WB_CASC_MAX_DEPTH == 3, "a case per depth");
    wb_set_error("cascade: no kernel for depth %d, rows-per-wave %d x %d waves", depth, rpw, waves);
    return WB_ERR_UNSUPPORTED;
}

// the diagnostic switches of wb_cascade_launch, read from the environment once
struct CascEnv {
    int dbg = 0;                    // WB_CASC_DBG
    int spar[4] = {32, 8, 16, 2};   // WB_CASC_SPAR: a wave flips to the stage-parallel tail when few windows are left (measured flat around these)
    int spar_wg = 32;               // WB_CASC_SPAR_WG
    size_t xlds = 0;                // WB_CASC_XLDS: more dynamic LDS = fewer workgroups per CU
    bool jit_off = false;           // WB_CASC_JIT=0: stay on the generic tile kernel
    CascEnv() {
        if (const char *e = getenv("WB_CASC_DBG")) dbg = atoi(e);
        if (const char *e = getenv("WB_CASC_SPAR")) sscanf(e, "%d,%d,%d,%d", &spar[0], &spar[1], &spar[2], &spar[3]);
        // the workgroup-wide re-count behind the segment [8, 16) takes every wave's queue as evaluated up to stage 16: a
        // wave must not leave run_segments for the tail before that stage (an override below 16 would skip stages 8..15)
        spar[0] = spar[0] < 16 ? 16 : spar[0];
        spar[2] = spar[2] < 16 ? 16 : spar[2];
        if (const char *e = getenv("WB_CASC_SPAR_WG")) spar_wg = atoi(e);
        if (const char *e = getenv("WB_CASC_XLDS")) xlds = (size_t)atoi(e);
        if (const char *e = getenv("WB_CASC_JIT")) jit_off = atoi(e) == 0;
    }
};

}  // namespace

int wb_keys_to_floats_launch(hipStream_t st, uint32_t *keys, int T) {
    if (T == 0) return WB_OK;
    hipLaunchKernelGGL(calib_keys_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, keys, T);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

int wb_cascade_group(int depth) { return depth >= 3 ? 2 : 4; }

bool wb_cascade_has_kernel(int depth, int rpw, int waves) {
    if (depth < 1 || depth > WB_CASC_MAX_DEPTH) return false;
#define WB_X(R, W) \
    if (rpw == R && waves == W) return true;
    WB_CASC_CONFIGS(WB_X)
#undef WB_X
    return false;
}

// dynamic LDS of the tile kernel in the layout of wb_cascade_tile.h; eb: 0 float32 tile, 1 bytes, 2 16-bit ranks
int wb_cascade_lds_bytes(int eb, int C, int rows, int pitch, int TR, int waves, int T, int lds_stages, int depth) {
    return (int)(wb_lds_stab_off(eb, C, rows, pitch, TR, T, waves) + (size_t)lds_stages * WB_STAGE_DWORDS(depth) * 4 + WB_LDS_CTL_BYTES);
}

int wb_cascade_prepare(int depth, int rpw, int waves) {
    return casc_dispatch(depth, rpw, waves, [](auto d, auto r, auto w) {
        constexpr int D = decltype(d)::value, R = decltype(r)::value, W = decltype(w)::value;
        for (const void *kernel : {reinterpret_cast<const void *>(&cascade_tile_kernel<D, R, W, 0>),
                                   reinterpret_cast<const void *>(&cascade_tile_kernel<D, R, W, 1>),
                                   reinterpret_cast<const void *>(&cascade_tile_kernel<D, R, W, 2>)})
            WB_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024));
        return WB_OK;
    });
}

extern "C" int wb_cascade_launch(void *stream, const WbModel *model, const void *chn, int chn_dtype,
                                 int64_t chn_stride, int batch, const WbLevel *levels, int n_levels,
                                 const WbTile *tiles, int n_tiles, WbDet *det, uint32_t *det_count,
                                 uint32_t shard_capacity, uint32_t *alive) {
    return wb_cascade_launch_z(stream, model, chn, chn_dtype, chn_stride, batch, levels, n_levels, tiles, n_tiles, det, det_count,
                               shard_capacity, alive, nullptr, 0);
}

extern "C" int wb_cascade_launch_z(void *stream, const WbModel *model, const void *chn, int chn_dtype,
                                   int64_t chn_stride, int batch, const WbLevel *levels, int n_levels,
                                   const WbTile *tiles, int n_tiles, WbDet *det, uint32_t *det_count,
                                   uint32_t shard_capacity, uint32_t *alive, uint32_t *zero, int zero_words) {
    WB_REQUIRE(zero_words == 0 || (zero && zero_words > 0), "wb_cascade_launch_z: zero_words without a pointer");
    WB_REQUIRE(model && chn && levels && tiles && det_count, "wb_cascade_launch: null pointer");
    WB_REQUIRE(det || shard_capacity == 0, "wb_cascade_launch: det is null but capacity > 0");
    WB_REQUIRE(batch >= 1 && batch <= 65535, "wb_cascade_launch: batch %d out of range", batch);
    WB_REQUIRE(n_levels >= 1 && n_tiles >= 1, "wb_cascade_launch: empty launch");
    WB_REQUIRE(chn_dtype == WB_DTYPE_F32 || chn_dtype == WB_DTYPE_U8 || chn_dtype == WB_DTYPE_RANK8 || chn_dtype == WB_DTYPE_RANK16,
               "wb_cascade_launch: channel dtype %d (float32, uint8 or ranks)", chn_dtype);
    CascArgs a;
    a.chn = chn;
    const int form = wb_tile_form(chn_dtype);
    const WbFormRecords &rec = model->form[form];
    a.chn_u8 = wb_form_elem_bytes(form);                     // element bytes of a byte tile
    a.chn_stride = chn_stride;
    a.levels = levels;
    a.tiles = tiles;
    a.n_levels = n_levels;
    // WB_DTYPE_RANK8: the bytes are threshold ranks of this model (wb_channels_launch wrote them): the uint8 tile
    // kernel with the rank records
    WB_REQUIRE(form != WB_FORM_RANK8 || rec.present, "wb_cascade_launch: this model has no rank tables (wb_model_info: rank_ok)");
    WB_REQUIRE(form != WB_FORM_RANK16 || rec.present, "wb_cascade_launch: this model has no 16-bit rank tables (wb_model_info: rank16_ok)");
    a.stages = rec.stages_dev;
    a.T = model->n_stages;
    a.m = model->m;
    a.n = model->n;
    a.C = model->C;
    a.lds_rows = rec.lds_rows;
    a.tile_unit = model->tile_rows;
    a.lds_pitch = model->lds_pitch;
    a.lds_stages = model->lds_stages;
    a.det = det;
    a.det_count = det_count;
    a.det_cap = shard_capacity;
    a.alive = alive;
    a.zero = zero;
    a.zero_words = zero_words;
    a.n_tiles = n_tiles;
    static const CascEnv env;
    a.dbg = env.dbg;
    for (int i = 0; i < 4; ++i) a.spar[i] = env.spar[i];
    a.spar_wg = env.spar_wg;
    dim3 grid((unsigned)n_tiles, (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (model->generic) {
        const GenArgs g = {flat_model(model), chn, a.chn_u8, chn_stride, levels, tiles, n_levels, n_tiles,
                           det, det_count, shard_capacity, alive, zero, zero_words};
        size_t lds = (((size_t)g.model.T * 4 + 15) & ~(size_t)15) + 256 * 8;
        WB_REQUIRE(lds <= 64 * 1024, "wb_cascade_launch: %d stages exceed the generic kernel's LDS", g.model.T);
        hipLaunchKernelGGL(cascade_generic_kernel, grid, dim3(256), lds, st, g);
        WB_HIP_CHECK(hipGetLastError());
        return WB_OK;
    }
    const size_t lds = (size_t)rec.lds_bytes + env.xlds;
    // the model-specialised kernel, when wb_model_specialize has built one for this kind of byte tile
    if (void *jf = !env.jit_off && !model->jit_off ? rec.jit : nullptr) {
        const int32_t *stages = a.stages;
        void *params[] = {&a, &stages};
        WB_HIP_CHECK(hipModuleLaunchKernel((hipFunction_t)jf, grid.x, grid.y, 1, (unsigned)model->waves * 64, 1, 1, (unsigned)lds, st,
                                           params, nullptr));
        return WB_OK;
    }
    return casc_dispatch(model->depth, rec.rpw, model->waves, [&](auto d, auto r, auto w) {
        constexpr int D = decltype(d)::value, R = decltype(r)::value, W = decltype(w)::value;
        if (a.chn_u8 == 2)
            hipLaunchKernelGGL((cascade_tile_kernel<D, R, W, 2>), grid, dim3(W * 64), lds, st, a, a.stages);
        else if (a.chn_u8)
            hipLaunchKernelGGL((cascade_tile_kernel<D, R, W, 1>), grid, dim3(W * 64), lds, st, a, a.stages);
        else
            hipLaunchKernelGGL((cascade_tile_kernel<D, R, W, 0>), grid, dim3(W * 64), lds, st, a, a.stages);
        WB_HIP_CHECK(hipGetLastError());
        return WB_OK;
    });
}

extern "C" int wb_tree_eval_launch(void *stream, const void *X, int x_dtype, int u, int v, int C, const int32_t *rs,
                                   const int32_t *cs, int64_t n_pos, const uint8_t *feature,
                                   const float *threshold, const int8_t *left, const int8_t *right,
                                   const float *prediction, int n_nodes, float *out) {
    WB_REQUIRE(n_pos >= 0, "wb_tree_eval_launch: negative count");
    if (n_pos == 0) return WB_OK;
    WB_REQUIRE(X && rs && cs && feature && threshold && left && right && prediction && out,
               "wb_tree_eval_launch: null pointer");
    WB_REQUIRE(u > 0 && v > 0 && C > 0 && n_nodes > 0 && n_nodes <= 127, "wb_tree_eval_launch: bad shape");
    WB_REQUIRE(x_dtype == WB_DTYPE_F32 || x_dtype == WB_DTYPE_U8, "wb_tree_eval_launch: channel dtype %d (float32 or uint8)", x_dtype);
    const int64_t blocks = (n_pos + 255) / 256;
    WB_REQUIRE(blocks <= 0x7fffffff, "wb_tree_eval_launch: too many windows for one launch");
    hipLaunchKernelGGL(tree_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, X,
                       (int)(x_dtype == WB_DTYPE_U8), u, v, C, rs, cs, n_pos, feature, threshold, left, right, prediction, n_nodes, out);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_gather_samples_launch(void *stream, const void *X, int x_dtype, int u, int v, int C,
                                        const int32_t *rs, const int32_t *cs, int64_t n_pos, int m, int n, void *out) {
    WB_REQUIRE(n_pos >= 0, "wb_gather_samples_launch: negative count");
    if (n_pos == 0) return WB_OK;
    WB_REQUIRE(X && rs && cs && out, "wb_gather_samples_launch: null pointer");
    WB_REQUIRE(u > 0 && v > 0 && C > 0 && m > 0 && n > 0 && m <= u && n <= v, "wb_gather_samples_launch: bad shape");
    WB_REQUIRE(x_dtype == WB_DTYPE_F32 || x_dtype == WB_DTYPE_U8, "wb_gather_samples_launch: channel dtype %d (float32 or uint8)", x_dtype);
    WB_REQUIRE(n_pos <= 0x7fffffff, "wb_gather_samples_launch: too many samples for one launch");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_pos);
    const int esz = x_dtype == WB_DTYPE_U8 ? 1 : 4;
    const size_t px = (size_t)C * esz;                       // bytes per pixel
    const bool al16 = px % 16 == 0 && (reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const bool al4 = px % 4 == 0 && (reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(out)) % 4 == 0;
    if (al16)       // whole pixels as 16-byte vectors (float32 x 4 channels: one per pixel)
        hipLaunchKernelGGL((gather_samples_kernel<uint4>), grid, dim3(64), 0, st, (const uint4 *)X, v, n * (int)(px / 16), rs, cs, m,
                           (int)(px / 16), (uint4 *)out);
    else if (al4)
        hipLaunchKernelGGL((gather_samples_kernel<uint32_t>), grid, dim3(64), 0, st, (const uint32_t *)X, v, n * (int)(px / 4), rs, cs,
                           m, (int)(px / 4), (uint32_t *)out);
    else
        hipLaunchKernelGGL((gather_samples_kernel<uint8_t>), grid, dim3(64), 0, st, (const uint8_t *)X, v, n * (int)px, rs, cs, m,
                           (int)px, (uint8_t *)out);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_samples_predict_launch(void *stream, const WbModel *model, const void *X, int x_dtype,
                                         int64_t n_samples, float *H, uint8_t *mask) {
    WB_REQUIRE(n_samples >= 0, "wb_samples_predict_launch: negative count");
    if (n_samples == 0) return WB_OK;
    WB_REQUIRE(model && X && H && mask, "wb_samples_predict_launch: null pointer");
    WB_REQUIRE(x_dtype == WB_DTYPE_F32 || x_dtype == WB_DTYPE_U8, "wb_samples_predict_launch: sample dtype %d (float32 or uint8)", x_dtype);
    const int64_t blocks = (n_samples + 255) / 256;
    WB_REQUIRE(blocks <= 0x7fffffff, "wb_samples_predict_launch: too many samples for one launch");
    hipLaunchKernelGGL(samples_predict_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flat_model(model), X,
                       (int)(x_dtype == WB_DTYPE_U8), n_samples, H, mask);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_samples_trace_launch(void *stream, const WbModel *model, const void *X, int x_dtype, int64_t n_samples,
                                       int reject, float *trace, float *final, uint32_t *alive) {
    WB_REQUIRE(n_samples >= 0, "wb_samples_trace_launch: negative count");
    if (n_samples == 0) return WB_OK;
    WB_REQUIRE(model && X, "wb_samples_trace_launch: null pointer");
    WB_REQUIRE(trace || final || alive, "wb_samples_trace_launch: no output asked for");
    WB_REQUIRE(x_dtype == WB_DTYPE_F32 || x_dtype == WB_DTYPE_U8, "wb_samples_trace_launch: sample dtype %d (float32 or uint8)", x_dtype);
    WB_REQUIRE(reject == 0 || reject == 1, "wb_samples_trace_launch: reject %d (0 or 1)", reject);
    const int64_t blocks = (n_samples + 255) / 256;
    WB_REQUIRE(blocks <= 0x7fffffff, "wb_samples_trace_launch: too many samples for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (alive) WB_HIP_CHECK(hipMemsetAsync(alive, 0, ((size_t)model->n_stages + 1) * 4, st));
    const TraceArgs a = {flat_model(model), X, (int)(x_dtype == WB_DTYPE_U8), reject, n_samples, trace, final, alive};
    hipLaunchKernelGGL(samples_trace_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_calib_min_launch(void *stream, const WbModel *model, const void *X, int x_dtype, int64_t n_samples,
                                   float floor, float *stage_min, uint32_t *n_retained) {
    WB_REQUIRE(n_samples >= 0, "wb_calib_min_launch: negative count");
    WB_REQUIRE(model && stage_min && n_retained && (X || n_samples == 0), "wb_calib_min_launch: null pointer");
    WB_REQUIRE(x_dtype == WB_DTYPE_F32 || x_dtype == WB_DTYPE_U8, "wb_calib_min_launch: sample dtype %d (float32 or uint8)", x_dtype);
    const int64_t blocks = (n_samples + 255) / 256;
    WB_REQUIRE(blocks <= 0x7fffffff, "wb_calib_min_launch: too many samples for one launch");
    hipStream_t st = (hipStream_t)stream;
    const int T = model->n_stages;
    uint32_t *keys = reinterpret_cast<uint32_t *>(stage_min);
    // whatever the outputs held: all-ones keys (above every score's) and a zero count, behind earlier work on the stream
    if (T) WB_HIP_CHECK(hipMemsetAsync(keys, 0xFF, (size_t)T * 4, st));
    WB_HIP_CHECK(hipMemsetAsync(n_retained, 0, 4, st));
    if (n_samples) {
        const CalibArgs a = {flat_model(model), X, (int)(x_dtype == WB_DTYPE_U8), floor, n_samples, keys, n_retained};
        hipLaunchKernelGGL(calib_min_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
        WB_HIP_CHECK(hipGetLastError());
    }
    return wb_keys_to_floats_launch(st, keys, T);
}

extern "C" int wb_tree_apply_launch(void *stream, const void *X, int x_dtype, int64_t n_samples, int m, int n, int C,
                                    const uint8_t *feature, const float *threshold, const int8_t *left,
                                    const int8_t *right, int n_nodes, int32_t *node) {
    WB_REQUIRE(n_samples >= 0, "wb_tree_apply_launch: negative count");
    if (n_samples == 0) return WB_OK;
    WB_REQUIRE(X && feature && threshold && left && right && node, "wb_tree_apply_launch: null pointer");
    WB_REQUIRE(m > 0 && n > 0 && C > 0 && n_nodes > 0 && n_nodes <= 127, "wb_tree_apply_launch: bad shape");
    WB_REQUIRE(x_dtype == WB_DTYPE_F32 || x_dtype == WB_DTYPE_U8, "wb_tree_apply_launch: sample dtype %d (float32 or uint8)", x_dtype);
    const int64_t blocks = (n_samples + 255) / 256;
    WB_REQUIRE(blocks <= 0x7fffffff, "wb_tree_apply_launch: too many samples for one launch");
    hipLaunchKernelGGL(tree_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, X,
                       (int)(x_dtype == WB_DTYPE_U8), n_samples, m, n, C, feature, threshold, left, right, n_nodes, node);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

#ifdef WB_CASC_STAMPS
// Diagnostic build: mean microseconds between consecutive stamps over the first n_wg workgroups
// of the last cascade launch (s_memrealtime ticks at 100 MHz).
extern "C" int wb_debug_cascade_stamps(int n_wg, double *mean_us7, double *lifetime_us) {
    if (n_wg > WB_STAMP_WGS) n_wg = WB_STAMP_WGS;
    std::vector<unsigned long long> h((size_t)n_wg * WB_STAMP_SLOTS);
    WB_HIP_CHECK(hipDeviceSynchronize());
    WB_HIP_CHECK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_stamps), h.size() * 8));
    double acc[7] = {0}, life = 0;
    for (int w = 0; w < n_wg; ++w) {
        const unsigned long long *s = &h[(size_t)w * WB_STAMP_SLOTS];
        for (int k = 0; k < 7; ++k) acc[k] += (double)(s[k + 1] - s[k]);
        life += (double)(s[7] - s[0]);
    }
    for (int k = 0; k < 7; ++k) mean_us7[k] = acc[k] / n_wg / 100.0;
    *lifetime_us = life / n_wg / 100.0;
    return WB_OK;
}
#endif
