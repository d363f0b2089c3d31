// The cascade model handle (WbModel: wb_common.h) and the rank group.  wb_model_create does all its host work first --
// validation, tile geometry, rank tables, stage records per tile form (wb_stage_records.h), the diagnostic dump -- and then
// uploads; one routine frees a handle, whoever owns which part of it.
#include <stdlib.h>

#include "wb_common.h"

using namespace wb_records;

namespace {

// One block allocated and copied to the device per call; nothing more is tried after the first failure (`e` says which).
struct Upload {
    hipError_t e = hipSuccess;
    template <typename T> void operator()(T **dst, const void *src, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void **)dst, bytes ? bytes : 4);
        if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    }
};

template <typename T> T *host_copy(const T *src, size_t count) {
    T *p = static_cast<T *>(malloc(count * sizeof(T) + 4));
    if (count) memcpy(p, src, count * sizeof(T));
    return p;
}

// Everything a handle owns: its specialised kernels always, the stage tables and rank tables marked as its own, and -- unless
// it is a member view -- the node arrays and the host copy of the trees.  Then the handle itself.
void model_free(WbModel *model) {
    for (WbFormRecords &rec : model->form) {
        wb_jit_release(rec.jit);
        if (!rec.owned) continue;
        if (rec.stages_dev) (void)hipFree(rec.stages_dev);
        free(rec.stages_host);
    }
    for (WbRankTable &rt : model->ranks)
        if (rt.owned && rt.lut_dev) (void)hipFree(rt.lut_dev);
    if (!model->proxy) {
        void *h[] = {model->h_node_off, model->h_feature, model->h_threshold, model->h_prediction, model->h_left, model->h_right, model->h_theta};
        for (void *p : h) free(p);
        void *g[] = {model->g_node_off, model->g_feat, model->g_thr, model->g_left, model->g_right, model->g_pred, model->g_theta};
        for (void *p : g)
            if (p) (void)hipFree(p);
    }
    delete model;
}

// The cascade tile of a model: the largest (rpw * waves) x 64 windows whose float32 LDS footprint leaves two workgroups per
// CU; WB_CASC_RPW / WB_CASC_WAVES override the default for tuning.  Sets the geometry fields and every form's LDS bytes.
// The tile is chosen per form: a one-byte form (uint8 channels, 8-bit ranks) holds a quarter of the float32 tile's bytes
// per row and takes rows per wave of its own -- WB_CASC_BYTE_RPW, or WB_CASC_RPW as asked for (not halved by the float32
// budget) -- when the taller tile is a whole multiple of the model's, has a kernel, and leaves four workgroups per CU
// (40 KB of LDS); else the model's.  The float32 and the two-byte form keep the model's (at 64 rows: 91 KB, and 46 KB of tile).
void choose_geometry(WbModel *M) {
    const int budget = 80 * 1024, byte_budget = 40 * 1024, D = M->depth;
    int rpw = 4, waves = 8, byte_rpw = WB_CASC_BYTE_RPW;
    if (const char *e = getenv("WB_CASC_RPW")) byte_rpw = rpw = atoi(e);
    if (const char *e = getenv("WB_CASC_BYTE_RPW")) byte_rpw = atoi(e);
    if (const char *e = getenv("WB_CASC_WAVES")) waves = atoi(e);
    M->lds_pitch = WB_CASC_TC + M->n;   // tile row (64 + n - 1 pixels) + one pad column (spare slot of the tile load)
    M->lds_stages = (M->n_stages * WB_STAGE_DWORDS(D) * 4 <= 16 * 1024) ? M->n_stages : 0;
    M->stage_dwords = WB_STAGE_DWORDS(D);
    for (;; rpw >>= 1) {
        M->rpw = rpw;
        M->waves = waves;
        M->tile_rows = rpw * waves;
        M->lds_rows = M->tile_rows + M->m - 1;
        for (int f = 0; f < WB_FORM_COUNT; ++f) {
            M->form[f].elem_bytes = wb_form_elem_bytes(f);
            M->form[f].lds_bytes = wb_cascade_lds_bytes(M->form[f].elem_bytes, M->C, M->lds_rows, M->lds_pitch, M->tile_rows, waves,
                                                        M->n_stages, M->lds_stages, D);
        }
        if (M->form[WB_FORM_F32].lds_bytes <= budget || rpw <= 1) break;
    }
    for (int f = 0; f < WB_FORM_COUNT; ++f) {
        WbFormRecords &rec = M->form[f];
        rec.rpw = M->rpw;
        rec.tile_rows = M->tile_rows;
        rec.lds_rows = M->lds_rows;
        if (rec.elem_bytes != 1 || byte_rpw <= M->rpw || byte_rpw % M->rpw != 0 || !wb_cascade_has_kernel(D, byte_rpw, waves)) continue;
        const int tr = byte_rpw * waves, rows = tr + M->m - 1;
        const int lds = wb_cascade_lds_bytes(1, M->C, rows, M->lds_pitch, tr, waves, M->n_stages, M->lds_stages, D);
        if (lds > byte_budget) continue;
        rec.rpw = byte_rpw;
        rec.tile_rows = tr;
        rec.lds_rows = rows;
        rec.lds_bytes = lds;
    }
}

// the node arrays as the generic cascade kernel and the per-sample cascade (wb_samples_predict_launch) walk them, from the
// handle's host copy of the trees: every model carries them (a few KiB)
void upload_node_arrays(WbModel *M, Upload &up) {
    const size_t n_nodes = (size_t)M->n_nodes;
    std::vector<int32_t> feat(n_nodes), lft(n_nodes), rgt(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) {
        feat[i] = M->h_feature[i * 3] | (M->h_feature[i * 3 + 1] << 8) | (M->h_feature[i * 3 + 2] << 16);
        lft[i] = M->h_left[i];
        rgt[i] = M->h_right[i];
    }
    up(&M->g_node_off, M->h_node_off, ((size_t)M->n_stages + 1) * 4);
    up(&M->g_feat, feat.data(), n_nodes * 4);
    up(&M->g_thr, M->h_threshold, n_nodes * 4);
    up(&M->g_left, lft.data(), n_nodes * 4);
    up(&M->g_right, rgt.data(), n_nodes * 4);
    up(&M->g_pred, M->h_prediction, n_nodes * 4);
    up(&M->g_theta, M->h_theta, (size_t)M->n_stages * 4);
}

// WB_DUMP_STAGES=path (diagnostic): int32 {records, stage_dwords, depth, mask}, then the stage tables of the forms in the
// mask (bit f: form f), in the order of the forms
void dump_stages(const WbModel *M, int n_records, const std::vector<int32_t> *packs) {
    const char *path = getenv("WB_DUMP_STAGES");
    FILE *f = path ? fopen(path, "wb") : nullptr;
    if (!f) return;
    int32_t hdr[4] = {n_records, M->stage_dwords, M->depth, 0};
    for (int k = 0; k < WB_FORM_COUNT; ++k) hdr[3] |= M->form[k].present << k;
    fwrite(hdr, 4, 4, f);
    for (int k = 0; k < WB_FORM_COUNT; ++k)
        if (M->form[k].present) fwrite(packs[k].data(), 4, packs[k].size(), f);
    fclose(f);
}

// WB_DUMP_RANKS=path (diagnostic): for each rank form built, int32 {wide, K, slots, cells}, float k[4], float b[4], then
// the lut bytes (float S[4][slots], then base[4][cells]: uint8, wide: uint16); an empty file when none was built
void dump_ranks(const RankTables *const *rt, const int *wide, int n) {
    const char *path = getenv("WB_DUMP_RANKS");
    FILE *f = path ? fopen(path, "wb") : nullptr;
    if (!f) return;
    for (int i = 0; i < n; ++i) {
        const int32_t hdr[4] = {wide[i], rt[i]->K, wide[i] ? WB_BIN16_SLOTS : WB_BIN_SLOTS, wide[i] ? WB_BIN16_CELLS : WB_BIN_CELLS};
        fwrite(hdr, 4, 4, f);
        fwrite(rt[i]->k, 4, 4, f);
        fwrite(rt[i]->b, 4, 4, f);
        fwrite(rt[i]->lut.data(), 1, rt[i]->lut.size(), f);
    }
    fclose(f);
}

}  // namespace

extern "C" int wb_model_create(int n_stages, const int32_t *node_off, const uint8_t *feature,
                               const float *threshold, const int8_t *left, const int8_t *right,
                               const float *prediction, const float *theta, int m, int n, int C,
                               WbModel **out) {
    WB_REQUIRE(out, "wb_model_create: out is null");
    *out = nullptr;
    WB_REQUIRE(n_stages >= 0 && n_stages <= 16384, "wb_model_create: n_stages=%d out of range", n_stages);
    WB_REQUIRE(m >= 1 && n >= 1 && C >= 1 && m <= 256 && n <= 256 && C <= 256,
               "wb_model_create: window shape (%d,%d,%d) out of range (features are uint8)", m, n, C);
    WB_REQUIRE(n_stages == 0 || (node_off && feature && threshold && left && right && prediction && theta),
               "wb_model_create: null array");
    // ---- 1. the trees
    std::vector<TreeView> trees;
    int D = 1;
    int rc = validate_trees(n_stages, node_off, feature, threshold, left, right, prediction, m, n, C, trees, &D);
    if (rc != WB_OK) return rc;
    // deep trees, or windows whose LDS tile would not fit a CU: generic node-walk kernel
    const int min_lds = C * (4 + m - 1) * (WB_CASC_TC + n) * 4 + 4 * WB_CASC_TC * 8 + n_stages * 4;
    const bool generic = D > WB_CASC_MAX_DEPTH || min_lds > 150 * 1024 || getenv("WB_CASC_GENERIC") != nullptr;

    WbModel *M = new WbModel();
    M->n_stages = n_stages;
    M->depth = D;
    M->generic = generic ? 1 : 0;
    M->m = m;
    M->n = n;
    M->C = C;
    M->n_nodes = n_stages ? node_off[n_stages] : 0;
    // ---- 2. the geometry, 3. the rank tables, 4. the stage records of every form the model has, 5. the dump
    std::vector<int32_t> packs[WB_FORM_COUNT], rank[2];
    RankTables rt[2];
    if (generic) {
        // one thread per window, 4 x 64 windows per workgroup, features gathered from HBM/L2: no tile, no records
        M->rpw = 1;
        M->waves = 4;
        M->tile_rows = 4;
    } else {
        choose_geometry(M);
        if (M->form[WB_FORM_F32].lds_bytes > 160 * 1024) {
            wb_set_error("wb_model_create: window (%d,%d,%d) with %d stages needs %d B of LDS (> 160 KiB)", m, n, C,
                         n_stages, M->form[WB_FORM_F32].lds_bytes);
            delete M;
            return WB_ERR_UNSUPPORTED;
        }
        // rank tables for float32 channels: in one byte, and in two for cascades whose thresholds do not fit a byte's ranks --
        // both built for every model that qualifies (a few KiB); the engine uses the wider when the narrower is not there
        const bool want_ranks = C == 4 && n_stages > 0 && getenv("WB_NO_RANKS") == nullptr;
        std::vector<TreeView> ranked[2] = {trees, trees};
        M->form[WB_FORM_F32].present = M->form[WB_FORM_U8].present = 1;
        for (int w = 0; w < 2; ++w) {
            if (!want_ranks || !build_rank_tables({&trees}, rt[w], w == 1)) continue;
            rank[w].assign((size_t)M->n_nodes, -1);
            assign_ranks(ranked[w], node_off, rt[w], rank[w]);
            M->form[WB_FORM_RANK8 + w].present = M->ranks[w].owned = 1;
            M->ranks[w].iters = rt[w].K;
            for (int c = 0; c < 4; ++c) {
                M->ranks[w].k[c] = rt[w].k[c];
                M->ranks[w].b[c] = rt[w].b[c];
            }
        }
        const int G = wb_cascade_group(D);      // trailing no-op records
        M->stage_words = (size_t)(n_stages + G) * M->stage_dwords;
        for (int f = 0; f < WB_FORM_COUNT; ++f) {
            if (!M->form[f].present) continue;
            pack_stages(f, f >= WB_FORM_RANK8 ? ranked[f - WB_FORM_RANK8] : trees, theta, D, M->lds_rows, M->lds_pitch, C, M->stage_dwords,
                        G, packs[f]);
            M->form[f].owned = 1;
            if (f != WB_FORM_F32) M->form[f].stages_host = host_copy(packs[f].data(), packs[f].size());
        }
        dump_stages(M, n_stages + G, packs);
        const RankTables *built[2];
        int wide[2], n_built = 0;
        for (int w = 0; w < 2; ++w)
            if (M->form[WB_FORM_RANK8 + w].present) {
                built[n_built] = &rt[w];
                wide[n_built++] = w;
            }
        dump_ranks(built, wide, n_built);
    }
    // host copy of the trees as the caller gave them (wb_rankgroup_create)
    const int32_t zero = 0;
    M->h_node_off = host_copy(n_stages ? node_off : &zero, (size_t)n_stages + 1);
    M->h_feature = host_copy(feature, (size_t)M->n_nodes * 3);
    M->h_threshold = host_copy(threshold, (size_t)M->n_nodes);
    M->h_prediction = host_copy(prediction, (size_t)M->n_nodes);
    M->h_left = host_copy(left, (size_t)M->n_nodes);
    M->h_right = host_copy(right, (size_t)M->n_nodes);
    M->h_theta = host_copy(theta, (size_t)n_stages);
    // ---- 6. the uploads
    Upload up;
    upload_node_arrays(M, up);
    if (up.e != hipSuccess) {
        wb_set_error("wb_model_create: uploading the node arrays failed: %s", hipGetErrorString(up.e));
        model_free(M);
        return WB_ERR_HIP;
    }
    if (generic) {
        *out = M;
        return WB_OK;
    }
    for (int f = 0; f < WB_FORM_COUNT; ++f)
        if (M->form[f].present) up(&M->form[f].stages_dev, packs[f].data(), packs[f].size() * 4);
    for (int w = 0; w < 2; ++w)
        if (M->ranks[w].owned) up(&M->ranks[w].lut_dev, rt[w].lut.data(), rt[w].lut.size());
    if (up.e != hipSuccess) {
        wb_set_error("wb_model_create: uploading %zu stage bytes failed: %s", M->stage_words * 4, hipGetErrorString(up.e));
        model_free(M);
        return WB_ERR_HIP;
    }
    for (int f = 0; f < WB_FORM_COUNT && rc == WB_OK; ++f)
        if (f == WB_FORM_F32 || M->form[f].rpw != M->rpw) rc = wb_cascade_prepare(D, M->form[f].rpw, M->waves);
    if (rc != WB_OK) {
        model_free(M);
        return rc;
    }
    *out = M;
    return WB_OK;
}

extern "C" int wb_model_destroy(WbModel *model) {
    if (!model) return WB_OK;
    if (model->proxy) {
        wb_set_error("wb_model_destroy: this handle is a member view of a rank group (wb_rankgroup_destroy frees it)");
        return WB_ERR_INVALID;
    }
    model_free(model);
    return WB_OK;
}

extern "C" int wb_model_info(const WbModel *model, WbModelInfo *info) {
    WB_REQUIRE(model && info, "wb_model_info: null pointer");
    info->n_stages = model->n_stages;
    info->depth = model->depth;
    info->m = model->m;
    info->n = model->n;
    info->C = model->C;
    info->tile_rows = model->tile_rows;
    info->tile_cols = WB_CASC_TC;
    info->lds_bytes = model->form[WB_FORM_F32].lds_bytes;
    info->rank_ok = model->form[WB_FORM_RANK8].present;
    info->rank16_ok = model->form[WB_FORM_RANK16].present;
    info->specialized = 0;                       // bit 0 uint8, 1 ranks, 2 16-bit ranks
    for (int f = WB_FORM_U8; f < WB_FORM_COUNT; ++f) info->specialized |= (model->form[f].jit ? 1 : 0) << (f - WB_FORM_U8);
    return WB_OK;
}

// Window rows of the tile that wb_cascade_launch's kernel for `chn_dtype` covers per workgroup: wb_model_info's tile_rows
// or a multiple of it (choose_geometry).  A tile table for that form alone needs only the entries that start such a tile.
extern "C" int wb_model_form_rows(const WbModel *model, int chn_dtype, int *tile_rows, int *lds_bytes) {
    WB_REQUIRE(model && tile_rows, "wb_model_form_rows: null pointer");
    WB_REQUIRE(chn_dtype == WB_DTYPE_F32 || chn_dtype == WB_DTYPE_U8 || chn_dtype == WB_DTYPE_RANK8 || chn_dtype == WB_DTYPE_RANK16,
               "wb_model_form_rows: channel dtype %d (float32, uint8 or ranks)", chn_dtype);
    const WbFormRecords &rec = model->form[wb_tile_form(chn_dtype)];
    *tile_rows = model->generic ? model->tile_rows : rec.tile_rows;
    if (lds_bytes) *lds_bytes = model->generic ? 0 : rec.lds_bytes;
    return WB_OK;
}

// The same answer without a handle (and without a GPU): the tile wb_model_create would choose for a cascade of n_stages
// trees of `depth` on (m, n, C) windows, for channels of chn_dtype.  out = {rows per wave, waves, tile_rows, lds_bytes}.
extern "C" int wb_model_geometry(int n_stages, int depth, int m, int n, int C, int chn_dtype, int32_t *out) {
    WB_REQUIRE(out && n_stages >= 0 && depth >= 1 && depth <= WB_CASC_MAX_DEPTH && m >= 1 && n >= 1 && C >= 1, "wb_model_geometry: bad argument");
    WB_REQUIRE(chn_dtype == WB_DTYPE_F32 || chn_dtype == WB_DTYPE_U8 || chn_dtype == WB_DTYPE_RANK8 || chn_dtype == WB_DTYPE_RANK16,
               "wb_model_geometry: channel dtype %d (float32, uint8 or ranks)", chn_dtype);
    WbModel M = {};
    M.n_stages = n_stages;
    M.depth = depth;
    M.m = m;
    M.n = n;
    M.C = C;
    choose_geometry(&M);
    const WbFormRecords &rec = M.form[wb_tile_form(chn_dtype)];
    out[0] = rec.rpw;
    out[1] = M.waves;
    out[2] = rec.tile_rows;
    out[3] = rec.lds_bytes;
    return WB_OK;
}

// The loaded specialised kernels of a model off (0) or on (1) for wb_cascade_launch: off, the generic kernel scans -- what a
// caller needs to cross-check a specialised kernel on its own data (engine.py: _live_check), or to retire one it distrusts.
extern "C" int wb_model_use_specialized(WbModel *model, int enable) {
    WB_REQUIRE(model, "wb_model_use_specialized: null model");
    model->jit_off = enable ? 0 : 1;
    return WB_OK;
}

// The model-specialised kernel for one kind of byte tile (wb_jit.hip): compiled with hiprtc on first use (a couple of
// seconds), then taken from the process / disk cache, and trusted once it has passed its self-test (wb_jit_selftest).
// wb_cascade_launch uses it from then on for that channel dtype.
extern "C" int wb_model_specialize(WbModel *model, int chn_dtype) {
    WB_REQUIRE(model, "wb_model_specialize: null model");
    const int form = wb_tile_form(chn_dtype);
    if (form < WB_FORM_U8) {
        wb_set_error("wb_model_specialize: channel dtype %d has no specialised kernel (uint8 channels and threshold ranks do)", chn_dtype);
        return WB_ERR_UNSUPPORTED;
    }
    if (model->generic || model->n_stages == 0) {
        wb_set_error("wb_model_specialize: this model runs on the generic node-walk kernel (depth %d, %d stages)", model->depth, model->n_stages);
        return WB_ERR_UNSUPPORTED;
    }
    WbFormRecords &rec = model->form[form];
    if (!rec.present) {
        wb_set_error("wb_model_specialize: this model has no rank tables of that width (wb_model_info: rank_ok / rank16_ok)");
        return WB_ERR_UNSUPPORTED;
    }
    if (rec.jit) return WB_OK;
    if (rec.refused) {
        wb_set_error("wb_model_specialize: this model's specialised kernel failed its self-test earlier; it stays on the generic kernel");
        return WB_ERR_UNSUPPORTED;
    }
    int rc = wb_jit_get(rec.stages_host, model->stage_words, model->n_stages, model->depth, rec.rpw, model->waves, model->C,
                        rec.lds_rows, model->lds_pitch, rec.elem_bytes, model->lds_stages, &rec.jit);
    if (rc == WB_OK) {
        rc = wb_jit_selftest(model, chn_dtype, &rec);
        if (rc == WB_OK) return WB_OK;
        wb_jit_release(rec.jit);                           // (a build that is not used is idle: wb_jit.hip unloads idle modules when it holds too many)
        rec.jit = nullptr;
    }
    if (getenv("WB_JIT_VERBOSE")) fprintf(stderr, "[wb_jit] %s\n", wb_last_error());
    if (rc == WB_ERR_UNSUPPORTED) rec.refused = 1;         // (a compiler or HIP error is reported, not remembered)
    return rc;
}

// -------------------------------------------------------------------------------------------
// Several cascades scanning ONE pyramid of threshold ranks (reference waldboost/__init__.py:120-124: detect(image,
// *models) computes the channels once): the rank table of every channel is built from the UNION of the members'
// thresholds -- `v <= S_k  <=>  rank(v) <= k` holds for any sorted superset of a model's thresholds -- and every member
// gets stage records whose thresholds index that union.  A member is handed out as a VIEW of its model: a WbModel that
// shares its model's base (geometry, float32 and uint8 forms, node arrays) and has a WB_FORM_RANK8 form and specialised
// kernels of its own over the group's rank table, usable wherever a model is (wb_channels_launch's rank_model -- any
// member: they hold the same table --, wb_cascade_launch with WB_DTYPE_RANK8, wb_model_specialize, wb_model_info).
struct WbRankGroup {
    std::vector<WbModel *> views;
    uint8_t *lut_dev;
};

extern "C" int wb_rankgroup_destroy(WbRankGroup *g) {
    if (!g) return WB_OK;
    for (WbModel *v : g->views)
        if (v) model_free(v);
    if (g->lut_dev) (void)hipFree(g->lut_dev);
    delete g;
    return WB_OK;
}

extern "C" int wb_rankgroup_create(const WbModel *const *models, int n, WbRankGroup **out) {
    WB_REQUIRE(out, "wb_rankgroup_create: out is null");
    *out = nullptr;
    WB_REQUIRE(models && n >= 1 && n <= 64, "wb_rankgroup_create: 1..64 models");
    std::vector<std::vector<TreeView>> trees((size_t)n);
    std::vector<const std::vector<TreeView> *> sets;
    for (int i = 0; i < n; ++i) {
        const WbModel *m = models[i];
        WB_REQUIRE(m && !m->proxy, "wb_rankgroup_create: model %d is null or itself a member view", i);
        if (m->generic || m->C != 4 || m->n_stages == 0) {
            wb_set_error("wb_rankgroup_create: model %d has no rank form (node-walk kernel, %d channels, %d stages)", i, m->C, m->n_stages);
            return WB_ERR_UNSUPPORTED;
        }
        for (int s = 0; s < m->n_stages; ++s) {
            const int o = m->h_node_off[s];
            trees[i].push_back(TreeView{m->h_node_off[s + 1] - o, m->h_feature + (size_t)o * 3, m->h_threshold + o, m->h_left + o,
                                        m->h_right + o, m->h_prediction + o, nullptr});
        }
        sets.push_back(&trees[i]);
    }
    RankTables rt;
    const RankTables *built = &rt;
    const int narrow = 0;
    if (getenv("WB_NO_RANKS") != nullptr || !build_rank_tables(sets, rt)) {
        dump_ranks(&built, &narrow, 0);
        wb_set_error("wb_rankgroup_create: the models' thresholds do not fit one rank table (more than %d distinct per channel)", WB_BIN_MAX);
        return WB_ERR_UNSUPPORTED;
    }
    dump_ranks(&built, &narrow, 1);
    WbRankGroup *g = new WbRankGroup{std::vector<WbModel *>((size_t)n, nullptr), nullptr};
    Upload up;
    up(&g->lut_dev, rt.lut.data(), rt.lut.size());
    for (int i = 0; i < n && up.e == hipSuccess; ++i) {
        const WbModel *m = models[i];
        std::vector<int32_t> rank((size_t)m->n_nodes, -1), packed;
        assign_ranks(trees[i], m->h_node_off, rt, rank);
        pack_stages(WB_FORM_RANK8, trees[i], m->h_theta, m->depth, m->lds_rows, m->lds_pitch, m->C, m->stage_dwords,
                    wb_cascade_group(m->depth), packed);
        // the view: the model's base shared, nothing of it owned and no specialised kernel (one bakes the thresholds'
        // indices: per view) ...
        WbModel *v = new WbModel(*m);
        v->proxy = 1;
        v->jit_off = 0;
        for (WbFormRecords &rec : v->form) {
            rec.owned = rec.refused = 0;
            rec.jit = nullptr;
        }
        // ... its own rank8 form over the group's table, and no rank16 form (the member's 16-bit tables are not the union's)
        WbFormRecords &r8 = v->form[WB_FORM_RANK8];
        r8 = v->form[WB_FORM_U8];                            // (the byte tile: the same LDS and element bytes)
        r8.owned = 1;
        r8.stages_dev = nullptr;
        r8.stages_host = host_copy(packed.data(), packed.size());
        v->ranks[0] = WbRankTable{rt.K, {rt.k[0], rt.k[1], rt.k[2], rt.k[3]}, {rt.b[0], rt.b[1], rt.b[2], rt.b[3]}, g->lut_dev, 0};
        v->form[WB_FORM_RANK16] = WbFormRecords{};
        v->ranks[1] = WbRankTable{};
        g->views[(size_t)i] = v;
        up(&r8.stages_dev, packed.data(), packed.size() * 4);
    }
    if (up.e != hipSuccess) {
        wb_set_error("wb_rankgroup_create: uploading the tables failed: %s", hipGetErrorString(up.e));
        wb_rankgroup_destroy(g);
        return WB_ERR_HIP;
    }
    *out = g;
    return WB_OK;
}

extern "C" int wb_rankgroup_model(WbRankGroup *group, int i, WbModel **view) {
    WB_REQUIRE(group && view && i >= 0 && i < (int)group->views.size(), "wb_rankgroup_model: bad argument");
    *view = group->views[(size_t)i];
    return WB_OK;
}
