// The host side of a cascade model that needs no device: the four forms of a cascade tile, the canonical stage record, and
// the canonicalisation of the reference's flat-array decision trees into the complete-tree records the kernels read --
// validation, threshold rank tables, packing.  No HIP runtime call and no HIP header in here: a plain C++ program can
// include this file alone (it then defines wb_set_error itself).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/waldboost_hip.h"

// ---- error plumbing (thread-local message, never throws across the ABI; wb_api.hip) ----
void wb_set_error(const char *fmt, ...);

#define WB_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            wb_set_error(__VA_ARGS__);   \
            return WB_ERR_INVALID;       \
        }                                \
    } while (0)

// ---- the forms of a cascade tile: what the channel values a cascade scans are held as ----
enum WbTileForm {
    WB_FORM_F32 = 0,   // planar float32 tile
    WB_FORM_U8,        // uint8 channels: interleaved byte tile [row][col][C], integer thresholds
    WB_FORM_RANK8,     // threshold ranks of float32 channels, one byte (WB_DTYPE_RANK8): the byte tile, thresholds = ranks
    WB_FORM_RANK16,    // the same in two bytes (WB_DTYPE_RANK16): tile [row][col][C] of 16-bit elements
    WB_FORM_COUNT
};
// the form a channel dtype is scanned in (-1: none)
inline int wb_tile_form(int chn_dtype) {
    switch (chn_dtype) {
        case WB_DTYPE_F32: return WB_FORM_F32;
        case WB_DTYPE_U8: return WB_FORM_U8;
        case WB_DTYPE_RANK8: return WB_FORM_RANK8;
        case WB_DTYPE_RANK16: return WB_FORM_RANK16;
        default: return -1;
    }
}
// bytes of a tile element as the tile kernels count them (CascArgs::chn_u8, their EB parameter): 0 = planar float32
inline int wb_form_elem_bytes(int form) { return form == WB_FORM_F32 ? 0 : form == WB_FORM_RANK16 ? 2 : 1; }

// ---- cascade geometry ----
#define WB_CASC_TC 64        // windows per tile row = one per lane
#define WB_CASC_MAX_DEPTH 3
#define WB_BIN_MAX 254       // distinct thresholds per channel a binned tile can rank in one byte: ranks 0..254, 255 = NaN
                             // pixel; S[254] and S[255] of a channel's table are then always the +inf padding, so the
                             // channel kernel may read S[r] and S[r + 1] together for every rank r <= 254
#define WB_BIN_SLOTS 256     // entries of a channel's sorted threshold table
#define WB_BIN_CELLS 2048    // cells of a channel's lookup grid
#define WB_BIN_LUT_BYTES (4 * WB_BIN_SLOTS * 4 + 4 * WB_BIN_CELLS)   // float S[4][256], then uint8 base[4][N]
// ... and in two bytes (WB_DTYPE_RANK16): cascades with more distinct thresholds per channel than a byte ranks -- long soft
// cascades (reference __init__.py:230-269 appends stages without bound), deep trees.  The tables still live in LDS while
// a channel tile is ranked, so the count is bounded by that: 1020 thresholds per channel (S[1020..1023] = +inf padding: the
// channel kernel reads S[r .. r + 3] together), 512 grid cells with 16-bit base counts = 20 KiB.
#define WB_BIN16_MAX 1020
#define WB_BIN16_SLOTS 1024
#define WB_BIN16_CELLS 512
#define WB_BIN16_LUT_BYTES (4 * WB_BIN16_SLOTS * 4 + 4 * WB_BIN16_CELLS * 2)   // float S[4][1024], then uint16 base[4][512]

// The canonical stage record the cascade kernels read with scalar loads:
//   int   off[NI]   LDS byte offset of each internal node's feature (BFS order)
//   float thr[NI]
//   float pred[NL]  leaf predictions, left to right
//   float theta
// NI = 2^D - 1, NL = 2^D; padded to WB_STAGE_DWORDS(D) dwords.
#define WB_STAGE_NI(D) ((1 << (D)) - 1)
#define WB_STAGE_NL(D) (1 << (D))
#define WB_STAGE_DWORDS(D) ((((2 * WB_STAGE_NI(D) + WB_STAGE_NL(D) + 1) + 3) / 4) * 4)

// ---- canonicalisation: the caller's trees -> rank tables -> stage records ----
namespace wb_records {

struct TreeView {
    int k;  // nodes
    const uint8_t *feature;
    const float *threshold;
    const int8_t *left, *right;
    const float *prediction;
    const int32_t *rank;   // rank forms: index of the node's threshold among its channel's sorted distinct thresholds (-1: NaN)
};

// cell of the linear lookup grid a value falls into -- the host mirror of wb_bin_cell() in wb_common.h
// (fmaf is correctly rounded on both sides, so both map every float to the same cell)
inline uint32_t bin_cell(float v, float k, float b, int N) {
    const float q = fmaf(v, k, b);
    if (!(q > 0.0f)) return 0u;
    if (q >= (float)(N - 1)) return (uint32_t)(N - 1);
    return (uint32_t)q;
}

inline int tree_depth(const TreeView &t, int node) {
    if (t.left[node] < 0) return 0;
    int dl = tree_depth(t, t.left[node]), dr = tree_depth(t, t.right[node]);
    return 1 + (dl > dr ? dl : dr);
}

// The trees of a cascade as views of the caller's arrays, validated the way the reference walks them (training.py:84-96);
// *depth: the deepest of them (at least 1)
inline int validate_trees(int n_stages, const int32_t *node_off, const uint8_t *feature, const float *threshold, const int8_t *left,
                          const int8_t *right, const float *prediction, int m, int n, int C, std::vector<TreeView> &trees, int *depth) {
    int D = 1;
    trees.assign((size_t)n_stages, TreeView{});
    for (int s = 0; s < n_stages; ++s) {
        int o = node_off[s], k = node_off[s + 1] - node_off[s];
        WB_REQUIRE(o >= 0 && k >= 1 && k <= 127, "wb_model_create: stage %d has %d nodes (1..127 allowed: int8 links)", s, k);
        TreeView t{k, feature + (size_t)o * 3, threshold + o, left + o, right + o, prediction + o, nullptr};
        for (int i = 0; i < k; ++i) {
            if (t.left[i] < 0) continue;
            WB_REQUIRE(t.left[i] > i && t.left[i] < k && t.right[i] > i && t.right[i] < k,
                       "wb_model_create: stage %d node %d: children (%d,%d) must satisfy parent < child < %d",
                       s, i, (int)t.left[i], (int)t.right[i], k);
            WB_REQUIRE(t.feature[i * 3] < m && t.feature[i * 3 + 1] < n && t.feature[i * 3 + 2] < C,
                       "wb_model_create: stage %d node %d: feature (%d,%d,%d) outside window (%d,%d,%d)", s, i,
                       (int)t.feature[i * 3], (int)t.feature[i * 3 + 1], (int)t.feature[i * 3 + 2], m, n, C);
        }
        int d = tree_depth(t, 0);
        if (d > D) D = d;
        trees[s] = t;
    }
    *depth = D;
    return WB_OK;
}

// Fill the complete depth-D tree rooted at canonical node `ci` (BFS numbering: children of i are
// 2i+1, 2i+2) from reference node `node`.  A reference leaf above depth D becomes a dummy split
// (feature offset 0, both subtrees = that leaf), which cannot change the leaf value reached.
// WB_FORM_F32: offsets address the planar float32 tile [C][rows][pitch], thresholds are the model's floats.
// WB_FORM_U8: offsets address the interleaved byte tile [row][col][C], thresholds are integers (stored in the float
// slots): for an integer pixel v, `v <= thr` is `v <= floor(thr)`; a NaN or negative threshold is never met (-1), anything
// from 255 up always (255).
// WB_FORM_RANK8: the byte tile holds threshold ranks of float32 pixels: the integer is the node's rank.
// WB_FORM_RANK16: the same with 16-bit ranks: byte offsets into a tile of two-byte elements.
inline void fill(int form, const TreeView &t, int node, int ci, int d, int D, int rows, int pitch, int C, int32_t *off, float *thr,
                 float *pred) {
    const int NI = (1 << D) - 1;
    if (d == D) {
        pred[ci - NI] = t.prediction[node];
        return;
    }
    if (t.left[node] < 0) {
        off[ci] = 0;
        thr[ci] = 0.0f;
        fill(form, t, node, 2 * ci + 1, d + 1, D, rows, pitch, C, off, thr, pred);
        fill(form, t, node, 2 * ci + 2, d + 1, D, rows, pitch, C, off, thr, pred);
        return;
    }
    int fr = t.feature[node * 3 + 0], fc = t.feature[node * 3 + 1], ch = t.feature[node * 3 + 2];
    if (form == WB_FORM_F32) {
        off[ci] = ((ch * rows + fr) * pitch + fc) * 4;   // byte offset inside the LDS tile
        thr[ci] = t.threshold[node];
    } else {
        off[ci] = ((fr * pitch + fc) * C + ch) * wb_form_elem_bytes(form);
        const float th = t.threshold[node];
        int32_t ti = !(th >= 0.0f) ? -1 : (th >= 255.0f ? 255 : (int32_t)floorf(th));
        if (form != WB_FORM_U8) ti = t.rank[node];
        memcpy(&thr[ci], &ti, 4);
    }
    fill(form, t, t.left[node], 2 * ci + 1, d + 1, D, rows, pitch, C, off, thr, pred);
    fill(form, t, t.right[node], 2 * ci + 2, d + 1, D, rows, pitch, C, off, thr, pred);
}

// Rank tables of a SET of cascades (one model, or the members of a WbRankGroup): per channel the sorted distinct
// thresholds of every internal node, the linear cell grid over them and the per-cell base counts (wb_common.h).
struct RankTables {
    std::vector<float> S[4];
    float k[4], b[4];
    int K = 1;
    std::vector<uint8_t> lut;      // float S[4][slots], then base[4][cells]: uint8 (narrow) or uint16 (wide)
};

// wide: the 16-bit form (WB_BIN16_*: up to 1020 thresholds per channel, 512 cells, uint16 base counts)
inline bool build_rank_tables(const std::vector<const std::vector<TreeView> *> &sets, RankTables &rt, bool wide = false) {
    const int N = wide ? WB_BIN16_CELLS : WB_BIN_CELLS, SLOTS = wide ? WB_BIN16_SLOTS : WB_BIN_SLOTS;
    const int MAXT = wide ? WB_BIN16_MAX : WB_BIN_MAX;
    for (const std::vector<TreeView> *trees : sets)
        for (const TreeView &t : *trees)
            for (int i = 0; i < t.k; ++i)
                if (t.left[i] >= 0 && t.threshold[i] == t.threshold[i]) {
                    if (t.feature[i * 3 + 2] >= 4) return false;
                    rt.S[t.feature[i * 3 + 2]].push_back(t.threshold[i]);
                }
    for (int c = 0; c < 4; ++c) {
        std::sort(rt.S[c].begin(), rt.S[c].end());
        rt.S[c].erase(std::unique(rt.S[c].begin(), rt.S[c].end()), rt.S[c].end());     // (== merges -0.0 and 0.0)
        if ((int)rt.S[c].size() > MAXT) return false;
    }
    rt.lut.assign((size_t)4 * SLOTS * 4 + (size_t)4 * N * (wide ? 2 : 1), 0);
    float *Stab = reinterpret_cast<float *>(rt.lut.data());
    uint8_t *base8 = rt.lut.data() + (size_t)4 * SLOTS * 4;
    uint16_t *base16 = reinterpret_cast<uint16_t *>(base8);
    rt.K = 1;
    const int KMAX = wide ? 64 : 16;
    for (int c = 0; c < 4; ++c) {
        // the grid spans [lo, hi] of the channel's finite thresholds -- or, when a few far-out thresholds (1e30 next to
        // values around 10) would squeeze all the others into one cell, a trimmed range: whatever lies outside lands in
        // the two end cells (cell() clamps; it stays non-decreasing in v for any k > 0, which is all the ranks need)
        std::vector<float> fin;
        for (float v : rt.S[c])
            if (isfinite(v)) fin.push_back(v);
        std::vector<int> cnt((size_t)N, 0);
        const double trims[] = {0.0, 0.01, 0.03, 0.1, 0.25};
        bool placed = false;
        for (double q : trims) {
            float lo = INFINITY, hi = -INFINITY;
            if (!fin.empty()) {
                const size_t n = fin.size(), cut = (size_t)(q * (double)n);
                lo = fin[cut < n ? cut : n - 1];
                hi = fin[n - 1 - (cut < n ? cut : n - 1)];
                if (hi < lo) { const float t = lo; lo = hi; hi = t; }
            }
            double k = 1.0, b = 1.0;
            if (hi > lo) k = (double)(N - 2) / ((double)hi - (double)lo);
            if (lo <= hi) b = 1.0 - (double)lo * k;
            rt.k[c] = (float)k;
            rt.b[c] = (float)b;
            if (!(isfinite(rt.k[c]) && isfinite(rt.b[c]) && rt.k[c] > 0.0f)) continue;
            std::fill(cnt.begin(), cnt.end(), 0);
            int worst = 0;
            for (float v : rt.S[c]) {
                const int at = ++cnt[bin_cell(v, rt.k[c], rt.b[c], N)];    // non-decreasing in v
                worst = at > worst ? at : worst;
            }
            if (worst <= KMAX) { placed = true; break; }
        }
        if (!placed) return false;
        int run = 0;
        for (int j = 0; j < N; ++j) {
            if (wide)
                base16[(size_t)c * N + j] = (uint16_t)run;
            else
                base8[(size_t)c * N + j] = (uint8_t)run;
            run += cnt[j];
            if (cnt[j] > rt.K) rt.K = cnt[j];
        }
        for (int j = 0; j < SLOTS; ++j) Stab[c * SLOTS + j] = j < (int)rt.S[c].size() ? rt.S[c][j] : INFINITY;
    }
    return rt.K <= KMAX;
}

// rank[node] = index of the node's threshold in its channel's table (-1: leaf or NaN threshold); sets TreeView::rank
inline void assign_ranks(std::vector<TreeView> &trees, const int32_t *node_off, const RankTables &rt, std::vector<int32_t> &rank) {
    for (size_t s = 0; s < trees.size(); ++s) {
        for (int i = 0; i < trees[s].k; ++i) {
            const float th = trees[s].threshold[i];
            if (trees[s].left[i] < 0 || th != th) continue;
            const std::vector<float> &v = rt.S[trees[s].feature[i * 3 + 2]];
            rank[(size_t)node_off[s] + i] = (int32_t)(std::lower_bound(v.begin(), v.end(), th) - v.begin());
        }
        trees[s].rank = rank.data() + node_off[s];
    }
}

// The stage records of a cascade for one tile form (the rank forms: trees that assign_ranks has been through):
// (n_stages + G) records of SD dwords, the last G of them no-ops (offset 0, prediction 0, theta -inf) so that a group
// load never leaves the table
inline void pack_stages(int form, const std::vector<TreeView> &trees, const float *theta, int D, int rows, int pitch, int C, int SD,
                        int G, std::vector<int32_t> &packed) {
    const int NI = (1 << D) - 1, NL = 1 << D, n_stages = (int)trees.size();
    packed.assign((size_t)(n_stages + G) * SD, 0);
    for (int s = n_stages; s < n_stages + G; ++s) reinterpret_cast<float *>(packed.data() + (size_t)s * SD)[2 * NI + NL] = -INFINITY;
    for (int s = 0; s < n_stages; ++s) {
        int32_t *rec = packed.data() + (size_t)s * SD;
        fill(form, trees[s], 0, 0, 0, D, rows, pitch, C, rec, reinterpret_cast<float *>(rec + NI), reinterpret_cast<float *>(rec + 2 * NI));
        reinterpret_cast<float *>(rec)[2 * NI + NL] = theta[s];
    }
}

}  // namespace wb_records
