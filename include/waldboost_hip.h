/*
 * waldboost_hip.h -- C ABI of the MI355X (gfx950) waldboost detection hot path.
 *
 * The reference (RomanJuranek/waldboost) is pure Python and has no FFI/plugin
 * seam: the hot path sits behind plain Python calls.  This ABI is the seam the
 * build puts *beneath* that Python surface; each entry point names the
 * reference code it replaces.  All pointers marked "dev" are device pointers
 * supplied by the caller (e.g. torch ``data_ptr()``); no entry point allocates
 * result memory, synchronises the device, or throws.  Every function returns
 * WB_OK (0) or a negative error code; wb_last_error() gives the thread-local
 * message.  ``stream`` is a hipStream_t passed as void* (NULL = default stream).
 *
 *   reference waldboost/channels.py:93-101 (_image_octaves) + :55-64 (avg_pool_2)
 *        -> wb_octaves_launch
 *   reference waldboost/channels.py:111-146 (channel_pyramid: resize :132,
 *        grad_hist :40-52, gradients :16-21, avg_pool_2 :55-64, smooth :78-90)
 *        -> wb_channels_launch
 *   reference waldboost/fpga/channels.py:5-67 (grad_hist_4_u1, grad_mag_u1) and
 *        waldboost/channels.py:30-37 (grad_mag) as channel_opts["channels"]
 *        -> wb_channels_launch with channel_func = WB_CHN_*
 *   reference waldboost/channels.py:40-52, :30-37 called directly with non-default arguments
 *        -> wb_grad_hist_launch, wb_grad_mag_launch
 *   reference waldboost/model.py:62-67,272-283 (Model ctor/append) +
 *        waldboost/training.py:24-31 (DTree.__init__)
 *        -> wb_model_create / wb_model_destroy / wb_model_info
 *   reference waldboost/model.py:216-259 (Model.predict_on_image) +
 *        waldboost/training.py:84-96 (DTree.predict_on_image)
 *        -> wb_cascade_launch
 *   reference waldboost/training.py:84-96 called on explicit (rs, cs) lists
 *        -> wb_tree_eval_launch
 *   reference waldboost/model.py:136-147 (Model.get_boxes)
 *        -> wb_boxes_launch
 *   reference waldboost/model.py:173-179 (Model.detect: per-level results concatenated for the caller)
 *        -> wb_det_pack_launch
 *   reference waldboost/model.py:136-147 + :173-179 (get_boxes on the concatenated, ordered detections)
 *        -> wb_det_finish_launch; wb_det_finish_sorted_launch (the ordering on the device too);
 *           wb_det_order_batch_launch (the same per image of a batch)
 *   reference waldboost/samples.py:14-43 (gather_samples), waldboost/model.py:181-214 (Model.predict),
 *        waldboost/training.py:73-83 (DTree.apply/predict): the training-time callers of the hot path
 *        -> wb_gather_samples_launch, wb_samples_predict_launch, wb_tree_apply_launch
 *   reference waldboost/testing.py:46 (bbx.non_max_suppression on a detector's result) and
 *        scripts/waldboost-detect.py:36 (detect(..., iou_threshold=0.2, score_threshold=0, separate=False))
 *        -> wb_nms_launch, wb_nms_ordered_launch; wb_nms_finish_launch (on the buffer wb_det_finish_sorted_launch / wb_det_order_batch_launch left)
 *   reference waldboost/fpga/training.py:15-57 (H, _fit_threshold, _find_split: the split search of fpga.DTree.fit) and
 *        :133-138 (the samples of a split node move to its children)
 *        -> wb_fit_level_launch, wb_fit_route_launch
 *   reference waldboost/training.py:33-50 (DTree.fit: scikit-learn's DecisionTreeClassifier(class_weight="balanced"),
 *        gini criterion, best splitter, on float32 samples): the sort of every feature column and the split search,
 *        routing and re-partitioning of one tree level
 *        -> wb_cart_sort_launch, wb_cart_level_launch
 *   reference waldboost/samples.py:46-216 (label_boxes, select_candidates, get_samples_from_image: hard-negative mining),
 *        for a scanned batch and with a stated selection rule in place of np.random.choice
 *        -> wb_mine_select_launch, wb_mine_gather_launch
 *   no reference counterpart (its thetas are fitted during training only, training.py fit_rejection_threshold): the
 *        running score of a sample after every stage and the pruning minimum, for threshold calibration
 *        -> wb_samples_trace_launch, wb_calib_min_launch
 *   no reference counterpart (the reference stops at non_max_suppression): the boxes NMS kept, each merged with the live
 *        boxes of its cluster and counted
 *        -> wb_vote_launch
 */
#ifndef WALDBOOST_HIP_H
#define WALDBOOST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WB_ABI_VERSION 8

#define WB_OK 0
#define WB_ERR_INVALID (-1)     /* bad argument / malformed model */
#define WB_ERR_HIP (-2)         /* a HIP runtime call failed */
#define WB_ERR_UNSUPPORTED (-3) /* valid input this build has no kernel for */

#define WB_DTYPE_U8 0
#define WB_DTYPE_F32 1
/* Channel buffers only: one byte per element holding the RANK of the float32 channel value among the distinct
 * thresholds a given model tests on that channel (the number of them below the value; 255 for NaN).  For that
 * model `v <= threshold` (training.py:92) is `rank(v) <= index(threshold)` for every float v, so the cascade
 * decides exactly as on the float32 channels while reading a quarter of the bytes.  Written by
 * wb_channels_launch(rank_model, rank), read by wb_cascade_launch(chn_dtype = WB_DTYPE_RANK8) with the SAME
 * model.  Available when the model has 4 channels and at most 254 distinct thresholds per channel
 * (WbModelInfo.rank_ok). */
#define WB_DTYPE_RANK8 2
/* The same in TWO bytes per element (ABI 7): for models with up to 1020 distinct thresholds per channel -- long soft
 * cascades (reference __init__.py:230-269 appends stages without bound), deep trees -- whose channels would otherwise
 * stay float32.  65535 marks a NaN pixel.  Written by wb_channels_launch_x(rank_dtype = WB_DTYPE_RANK16), read by
 * wb_cascade_launch(chn_dtype = WB_DTYPE_RANK16); available when WbModelInfo.rank16_ok. */
#define WB_DTYPE_RANK16 13
/* Image buffers only: the other dtypes the reference's channel_pyramid accepts (channels.py:122 keeps
 * image.dtype).  All of them are held as float64 elements (exact for these integer types); the code tells the
 * octave kernel how avg_pool_2's adds wrap (integers wrap modulo 2^bits in the array's dtype, channels.py:61-64)
 * and the channel kernel how the resize result is cast back (.astype(dtype), channels.py:132: truncation toward
 * zero for integers; float64 stays float64 and is rounded to float32 by grad_hist's astype("f")).
 * Their per-octave (min, max) keys are 64-bit: minmax is then uint64 [batch][n_oct][2]. */
#define WB_DTYPE_F64 3
#define WB_DTYPE_I8 4
#define WB_DTYPE_I16 5
#define WB_DTYPE_U16 6
#define WB_DTYPE_I32 7
#define WB_DTYPE_U32 8
/* int64 / uint64 images whose values are exact in float64 (|v| < 2^51: the caller checks; their 2x2 sums then neither
 * round nor wrap), bool images (NumPy adds bools with logical OR, so a pooled pixel is "any of the four"; the resize
 * result is cast back with != 0) and float16 images (every add of avg_pool_2 and the cast back round to binary16). */
#define WB_DTYPE_I64 9
#define WB_DTYPE_U64 10
#define WB_DTYPE_BOOL 11
#define WB_DTYPE_F16 12

/* Channel functions (channel_opts["channels"] of the reference) the channel kernel implements:
 *   WB_CHN_GRAD_HIST       waldboost.channels.grad_hist (n_bins=4)    4 x float32  channels.py:40-52
 *   WB_CHN_GRAD_HIST_4_U1  waldboost.fpga.grad_hist_4_u1              4 x uint8    fpga/channels.py:29-53
 *   WB_CHN_GRAD_MAG_U1     waldboost.fpga.grad_mag_u1                 1 x uint8    fpga/channels.py:56-67
 *   WB_CHN_GRAD_MAG        waldboost.channels.grad_mag (norm=5,eps=1e-3) 1 x float32 channels.py:30-37 */
#define WB_CHN_GRAD_HIST 0
#define WB_CHN_GRAD_HIST_4_U1 1
#define WB_CHN_GRAD_MAG_U1 2
#define WB_CHN_GRAD_MAG 3

/* Channel images are [u][v][C] everywhere (the layout channel_pyramid hands to callers), in the
 * dtype the channel function produces (float32 or uint8): with C = 4 a pixel is one aligned
 * float4 (or one dword), so the channel kernel stores one vector per lane and a cascade tile row
 * is one contiguous run in HBM.  Offsets and strides of channel buffers (WbLevel.chn_off,
 * chn_stride) count ELEMENTS of that dtype; every level starts on a multiple of 4 elements. */

#define WB_MAX_OCTAVES 24

/* Detection / work-queue buffers are split into WB_DET_SHARDS independent append regions, each
 * with its own counter, so that concurrent workgroups do not serialise on one atomic word:
 *   records of shard s : det[s*shard_capacity .. s*shard_capacity + min(count[s], shard_capacity))
 * A workgroup appends to shard (blockIdx.x % WB_DET_SHARDS). */
#define WB_DET_SHARDS 64

/* One pyramid level (reference channels.py:127-146).  Built on the host: the level
 * plan is Python-float arithmetic in the reference and stays there. */
typedef struct WbLevel {
    int32_t oct;      /* source octave index                                        */
    int32_t src_h;    /* octave base size                                           */
    int32_t src_w;
    int32_t nh;       /* resized size (multiple of shrink)                          */
    int32_t nw;
    int32_t u;        /* channel image size = nh/shrink, nw/shrink                  */
    int32_t v;
    int32_t tap_off;  /* first entry of this level's resampling taps in the WbTap table:
                         nh row taps, then nw column taps                           */
    int64_t src_off;  /* element offset of the octave in the per-image octave buffer;
                         octave 0 lives in the image buffer itself (src_off unused) */
    int64_t chn_off;  /* float offset of this level in the per-image channel buffer */
    double sy;        /* zoom step src_h/nh (fp64 division, as scipy zoom does)     */
    double sx;        /* src_w/nw                                                   */
} WbLevel;            /* 64 bytes */

/* One axis of the order-1 resample of an output coordinate k (scipy.ndimage.zoom, grid_mode=True,
 * mode='mirror' -- what skimage.transform.resize runs for channels.py:132), built on the host in
 * fp64 exactly as NI_ZoomShift does: cc = ((k + 0.5) * step) - 0.5; i0 = floor(cc);
 * w0 = 1 - (cc - i0); w1 = 1 - w0; i1 = i0 + 1; indices mirror-mapped into the source. */
typedef struct WbTap {
    int32_t i0, i1;
    double w0, w1;
} WbTap; /* 24 bytes */

/* One workgroup's tile: level index + tile coordinates (in tiles). */
typedef struct WbTile {
    int32_t level;
    uint16_t ty;
    uint16_t tx;
} WbTile; /* 8 bytes */

/* One detection: window (r, c) of pyramid level `level` of image `image`
 * survived every stage with accumulated response `score` (model.py:255-259). */
typedef struct WbDet {
    int32_t image;
    int32_t level;
    uint16_t r;
    uint16_t c;
    float score;
} WbDet; /* 16 bytes */

typedef struct WbModel WbModel; /* opaque */

typedef struct WbModelInfo {
    int32_t n_stages;
    int32_t depth;      /* depth of the canonical complete trees the kernels walk  */
    int32_t m, n, C;    /* window shape (rows, cols, channels)                     */
    int32_t tile_rows;  /* cascade tile: tile_rows x 64 windows, the unit of WbTile.ty (wb_model_form_rows) */
    int32_t tile_cols;
    int32_t lds_bytes;  /* dynamic LDS per workgroup of the cascade kernel         */
    int32_t rank_ok;    /* 1 = the model has rank tables (WB_DTYPE_RANK8 channels)  */
    int32_t specialized; /* bit 0: a model-specialised kernel is loaded for uint8 channels, bit 1: for ranks, bit 2: for 16-bit ranks */
    int32_t rank16_ok;   /* 1 = the model has 16-bit rank tables (WB_DTYPE_RANK16 channels) */
} WbModelInfo;

int wb_abi_version(void);
const char *wb_last_error(void);

/* Tile sizes of the channel kernel (outputs per workgroup) for a channel function (WB_CHN_*) and shrink: what the
 * tile table handed to wb_channels_launch must be cut to. */
int wb_channels_tile(int channel_func, int shrink, int *tile_u, int *tile_v);

/* Channel count and element dtype (WB_DTYPE_*) a channel function produces. */
int wb_channel_func_info(int channel_func, int *n_channels, int *chn_dtype);

/* Octave pyramid of the raw image + per-octave min/max (the clip range of the resize).
 *   img      dev  [batch][H][W] of dtype, image b at img + b*img_stride elements
 *   oct      dev  per-image octave buffer for octaves 1..n_oct-1 (octave k at
 *                 oct + b*oct_stride + oct_off[k]); oct_off is a HOST array of n_oct
 *                 element offsets (oct_off[0] ignored)
 *   minmax   dev  uint32 [batch][n_oct][2] order-preserving keys of (min, max); uint64 [batch][n_oct][2]
 *                 for WB_DTYPE_F64 and the integer codes.  ACCUMULATED into (atomic max): the caller zeroes it
 * uint8 pooling wraps mod 256 before the divide, as the reference does under NumPy
 * (SURVEY S2); float32 pooling is ((a+b)+c)+d then /4. */
int wb_octaves_launch(void *stream, const void *img, int dtype, int batch, int H, int W,
                      int64_t img_stride, void *oct, int64_t oct_stride, const int64_t *oct_off,
                      int n_oct, uint32_t *minmax);
/* The same, and the launch's first workgroup also zeroes zero[0 .. zero_words): accumulators a LATER kernel of the step
 * adds into (the cascade's shard counters and alive[] statistics) -- with wb_cascade_launch_z a step needs no memset
 * launch at all.  Nothing else may touch those words while this launch runs. */
int wb_octaves_launch_z(void *stream, const void *img, int dtype, int batch, int H, int W,
                        int64_t img_stride, void *oct, int64_t oct_stride, const int64_t *oct_off,
                        int n_oct, uint32_t *minmax, uint32_t *zero, int zero_words);

/* All levels of all images: bilinear resize (fp64) -> channel function (grad_hist: Sobel
 * gradients -> 4 oriented channels with fp64 projection) -> shrink -> 3x3 smooth, fused per tile.
 *   channel_func  WB_CHN_*; the uint8 functions take uint8 images only (WB_ERR_UNSUPPORTED otherwise)
 *   levels   dev  WbLevel[n_levels];  tiles dev WbTile[n_tiles] (tile = wb_channels_tile)
 *   taps     dev  WbTap table addressed by WbLevel.tap_off
 *   img/oct  as for wb_octaves_launch; both buffers must extend 16 bytes past their last element
 *            (source rows are fetched with 4-byte-aligned dword loads)
 *   cs_sn    HOST double[8]: cos(theta_k), k=0..3 then sin(theta_k) (channels.py:43-46); used by
 *            WB_CHN_GRAD_HIST only
 *   chn      dev  [u][v][C] per level in the channel function's dtype, image b at
 *                 chn + b*chn_stride, level l at + levels[l].chn_off (elements); NULL (with `rank`) = do not
 *                 write the float32 channels at all
 *   rank_model, rank   optional (WB_CHN_GRAD_HIST only): also write the channels as WB_DTYPE_RANK8 bytes for that
 *                 model, same [u][v][4] layout and element offsets, image b at rank + b*rank_stride; the buffer
 *                 must extend 16 bytes past its last element (the cascade's 16-byte group loads).  Model.detect
 *                 (model.py:149-179) needs nothing else: the float32 pyramid then never touches HBM */
int wb_channels_launch(void *stream, const void *img, int64_t img_stride, const void *oct,
                       int64_t oct_stride, int dtype, int batch, const WbLevel *levels, int n_levels,
                       const WbTile *tiles, int n_tiles, const uint32_t *minmax, int n_oct,
                       const WbTap *taps, int channel_func, int shrink, int smooth, const double *cs_sn,
                       void *chn, int64_t chn_stride, const WbModel *rank_model, uint8_t *rank,
                       int64_t rank_stride);

/* The same launch with a per-tile side table (ABI 7): patches = dev WbTilePatch[n_tiles], entry i for tiles[i] -- the
 * source patch that tile stages in LDS for its resample, as wb_channels_tile_patches computes it on the HOST from the
 * library's own tile geometry (the level plan and its tiles are host data anyway, channels.py:124-131).  With the table a
 * workgroup starts its patch loads right behind its tile record instead of behind four chains of fp64 arithmetic that
 * every workgroup of a level would repeat.  patches = NULL: exactly wb_channels_launch.  Results are identical either way. */
typedef struct WbTilePatch {
    int32_t r_lo;    /* first source row / column of the patch in the level's octave                               */
    int32_t c_lo;
    uint16_t rows;   /* source rows r_lo .. r_lo + rows - 1; 0 = this tile stages no patch (an identity level, an   */
    uint16_t bytes;  /* up-scale, a patch beyond the LDS budget): it takes the kernel's other paths                 */
    uint32_t pad;
} WbTilePatch;       /* 16 bytes */
int wb_channels_tile_patches(int channel_func, int shrink, int smooth, const WbLevel *levels_host, int n_levels,
                             const WbTile *tiles_host, int n_tiles, WbTilePatch *out_host);
int wb_channels_launch_x(void *stream, const void *img, int64_t img_stride, const void *oct,
                         int64_t oct_stride, int dtype, int batch, const WbLevel *levels, int n_levels,
                         const WbTile *tiles, int n_tiles, const uint32_t *minmax, int n_oct,
                         const WbTap *taps, int channel_func, int shrink, int smooth, const double *cs_sn,
                         void *chn, int64_t chn_stride, const WbModel *rank_model, uint8_t *rank,
                         int64_t rank_stride, const WbTilePatch *patches, int rank_dtype);
/* rank_dtype: WB_DTYPE_RANK8 (what wb_channels_launch writes) or WB_DTYPE_RANK16 -- `rank` is then uint16 [u][v][4] per
 * level (rank_stride and the level offsets count ELEMENTS, as for every channel buffer), 8-byte aligned. */

/* The pyramid around a channel function this library has no kernel for (channels.py:119,136 calls whatever callable
 * channel_opts["channels"] holds -- the caller runs it, between these two):
 *   wb_resize_level_launch  one level's resized image, cast back to the image dtype (channels.py:132): level_host = HOST
 *                           WbLevel of that level, minmax_host = HOST copy of the level's octave's (min, max) keys as
 *                           wb_octaves_launch left them (two 32-bit words; two 64-bit words for the float64-held dtypes),
 *                           img / oct / taps dev as for wb_channels_launch (batch 1); out dev [nh][nw] of uint8 / float32 /
 *                           float64 (the float64-held dtypes: the cast value, as a double)
 *   wb_pool_smooth_launch   avg_pool_2 (shrink = 2, channels.py:55-64) and smooth_image_3d (smooth = 1, :78-90) of the
 *                           callable's result in dev [H][W][C] uint8 or float32 -> out dev [H/shrink][W/shrink][C]; tmp =
 *                           dev scratch of the pooled size when both steps run */
int wb_resize_level_launch(void *stream, const void *img, const void *oct, int dtype, const WbLevel *level_host,
                           const uint32_t *minmax_host, const WbTap *taps, void *out);
int wb_pool_smooth_launch(void *stream, const void *in, int chn_dtype, int H, int W, int C, int shrink, int smooth, void *tmp,
                          void *out);

/* The channel functions called directly on one float32 image (the caller's image.astype("f")) WITH ARGUMENTS
 * (reference channels.py:40-52 grad_hist(image, n_bins, full, bias) and :30-37 grad_mag(image, norm, eps); with
 * their default arguments, and inside channel_pyramid, they run in wb_channels_launch).
 *   wb_grad_hist_launch  cs_sn HOST double[2*n_bins]: cos(theta_k) then sin(theta_k) of np.linspace(0, pi or 2*pi,
 *                        n_bins+1)[:-1]; wide = 0: bias is a float32 value (a Python scalar is one under NumPy-2
 *                        promotion), out dev float32 [H][W][n_bins]; wide = 1: bias is a float64 / int64 NumPy scalar --
 *                        |chns| - bias and everything after it are float64, out dev float64 [H][W][n_bins]
 *   wb_grad_mag_launch   n_taps = 0: the plain magnitude (norm None or <= 1); else taps HOST float32[n_taps] =
 *                        triangle_kernel(norm), scratch dev float32[2*H*W]; out dev float32 [H][W]; wide = 0: eps is a
 *                        float32 value, mag / (norm + eps) in float32; wide = 1: eps is a float64 NumPy scalar -- the
 *                        in-place `mag /= norm + eps` divides in float64 and rounds once to float32 */
int wb_grad_hist_launch(void *stream, const float *img, int H, int W, int n_bins, int full, double bias, int wide,
                        const double *cs_sn, void *out);
int wb_grad_mag_launch(void *stream, const float *img, int H, int W, int n_taps, const float *taps, double eps, int wide,
                       float *scratch, float *out);

/* Build the device-side cascade from the reference's tree arrays (all HOST pointers).
 *   node_off  int32[n_stages+1]  first node of each stage's tree in the flat arrays
 *   feature   uint8[n_nodes][3]  (row, col, channel) inside the window
 *   threshold float[n_nodes], left/right int8[n_nodes] (-1 on leaves), prediction float[n_nodes]
 *   theta     float[n_stages]    rejection thresholds, -inf = stage never rejects
 * Trees must have parent index < child index (the order the reference walks them in,
 * training.py:88).  Trees up to depth 3 run in the LDS-tiled kernel; deeper ones in a generic
 * node-walk kernel (correct, not tuned). */
int wb_model_create(int n_stages, const int32_t *node_off, const uint8_t *feature,
                    const float *threshold, const int8_t *left, const int8_t *right,
                    const float *prediction, const float *theta, int m, int n, int C,
                    WbModel **out);
int wb_model_destroy(WbModel *model);
int wb_model_info(const WbModel *model, WbModelInfo *info);

/* Compile (hiprtc, a couple of seconds the first time; afterwards from the cache directory $WB_JIT_CACHE, default
 * ~/.cache/waldboost_amd) and load the model-specialised tile kernel for one kind of byte tile: chn_dtype
 * WB_DTYPE_RANK8, WB_DTYPE_RANK16 or WB_DTYPE_U8.  The model's stage records -- feature offsets, thresholds (model.py:62-67,
 * training.py:24-31), leaf values and theta -- are compile-time constants in it.  wb_cascade_launch uses it from then
 * on for that dtype; results are bit-identical to the generic kernel's -- which the call verifies before it returns: the
 * new kernel and the generic one scan a synthetic pyramid of byte tiles (8,493 windows, six passes; $WB_JIT_SELFTEST) and
 * must agree on every per-stage alive count and detection record.  WB_ERR_UNSUPPORTED for float32 channels, for models on
 * the node-walk kernel, and for a model whose build does not pass that test; a failed compilation also leaves the model
 * on the generic kernel. */
int wb_model_specialize(WbModel *model, int chn_dtype);
/* ABI 8.  Make wb_cascade_launch ignore (enable = 0) or use again (1) the specialised kernels this model has loaded: with
 * them off the generic kernel scans.  For callers that cross-check a specialised kernel on their own data before they
 * rely on it (the Python engine does, on the image at hand, right after wb_model_specialize), or retire one. */
int wb_model_use_specialized(WbModel *model, int enable);
/* The tile of the kernel that scans channels of chn_dtype: *tile_rows window rows (x tile_cols) per workgroup, and its
 * dynamic LDS in *lds_bytes (may be NULL).  The rows are wb_model_info's tile_rows -- the float32 form's, and the unit of
 * WbTile.ty for every form -- or a whole multiple k of it: the one-byte forms (WB_DTYPE_U8, WB_DTYPE_RANK8) scan tiles
 * of 64 x 64 windows where 40 KB of LDS hold them.  Such a kernel serves the table entries whose ty is a multiple of k,
 * each for k units of rows, and its workgroups leave at once on the others: a table of every unit is right for every
 * form, and a table for one form may hold only the entries that start a tile. */
int wb_model_form_rows(const WbModel *model, int chn_dtype, int *tile_rows, int *lds_bytes);
/* The same without a handle or a GPU: the tile wb_model_create chooses for a cascade of n_stages trees of `depth` on
 * (m, n, C) windows, for channels of chn_dtype.  out[4] = {rows per wave, waves, tile_rows, lds_bytes}. */
int wb_model_geometry(int n_stages, int depth, int m, int n, int C, int chn_dtype, int32_t *out);

/* Several cascades over ONE pyramid of threshold ranks (waldboost.detect(image, *models), reference __init__.py:120-124:
 * the channels are computed once for all models): one rank table per channel from the UNION of the members'
 * thresholds.  wb_rankgroup_model hands out member i as a VIEW of its model -- a WbModel handle owned by the group that
 * shares everything with the model but the rank tables; pass any view as wb_channels_launch's rank_model (they hold
 * the same table) and view i to wb_cascade_launch(WB_DTYPE_RANK8) / wb_model_specialize / wb_model_info.  The models
 * must outlive the group.  WB_ERR_UNSUPPORTED when a channel's union exceeds 254 thresholds or a member has no rank
 * form (node-walk models, C != 4): scan float32 channels then. */
typedef struct WbRankGroup WbRankGroup;
int wb_rankgroup_create(const WbModel *const *models, int n, WbRankGroup **out);
int wb_rankgroup_model(WbRankGroup *group, int i, WbModel **view);
int wb_rankgroup_destroy(WbRankGroup *group);

/* Build check of the specialised kernel's source without a GPU: a synthetic cascade of n_stages depth-`depth` trees
 * through the generator and hiprtc for `arch` (e.g. "gfx950"); *code_bytes = size of the code object. */
int wb_jit_compile_check(int depth, int n_stages, const char *arch, int64_t *code_bytes);
/* The same for a tile of elem_bytes-wide elements (1: uint8 channels / WB_DTYPE_RANK8, 2: WB_DTYPE_RANK16). */
int wb_jit_compile_check2(int depth, int n_stages, int elem_bytes, const char *arch, int64_t *code_bytes);
/* The same with rpw window rows per wave on eight waves (4: the tile of 32 rows, 8: the one-byte forms' 64). */
int wb_jit_compile_check3(int depth, int n_stages, int elem_bytes, int rpw, const char *arch, int64_t *code_bytes);

/* Dense sliding-window cascade over all levels of all images.
 *   chn           [u][v][C] per level as written by wb_channels_launch (or caller-provided), of
 *                 chn_dtype WB_DTYPE_F32 or WB_DTYPE_U8 (uint8 values compare against the float32
 *                 thresholds as their exact float32 values, like NumPy's uint8 <= float32), or
 *                 WB_DTYPE_RANK8 (ranks of float32 channels for THIS model); a byte
 *                 buffer must extend 16 bytes past its last element (16-byte group loads)
 *   tiles         dev WbTile[n_tiles]: tiles of tile_rows x tile_cols WINDOWS over the
 *                 (u-m) x (v-n) window grid of each level; ty counts wb_model_info's
 *                 tile_rows for every chn_dtype (wb_model_form_rows: a form with taller tiles)
 *   det           dev WbDet[WB_DET_SHARDS][shard_capacity]; det_count dev uint32[WB_DET_SHARDS]:
 *                 survivors per shard (a count may exceed shard_capacity: the records beyond it
 *                 are dropped, the count stays exact -- grow the buffer and launch again)
 *   alive         dev uint32 [batch][n_levels][n_stages]: windows entering each stage (the reference's n_weak
 *                 is its sum, n_loc the sum of column 0: model.py:248,252); NULL = no statistics
 * det_count and alive are ACCUMULATED into: the caller zeroes them.  Record order is unspecified; sort by
 * (image, level, r, c) to obtain the reference order. */
int wb_cascade_launch(void *stream, const WbModel *model, const void *chn, int chn_dtype,
                      int64_t chn_stride, int batch, const WbLevel *levels, int n_levels,
                      const WbTile *tiles, int n_tiles, WbDet *det, uint32_t *det_count,
                      uint32_t shard_capacity, uint32_t *alive);
/* The same, and the launch's first workgroup also zeroes zero[0 .. zero_words): the octaves' (min, max) keys, which
 * nothing of this step reads any more once the channel kernel has finished -- ready for the next step's
 * wb_octaves_launch(_z). */
int wb_cascade_launch_z(void *stream, const WbModel *model, const void *chn, int chn_dtype,
                        int64_t chn_stride, int batch, const WbLevel *levels, int n_levels,
                        const WbTile *tiles, int n_tiles, WbDet *det, uint32_t *det_count,
                        uint32_t shard_capacity, uint32_t *alive, uint32_t *zero, int zero_words);

/* The valid records of all shards of a detection buffer (as wb_cascade_launch fills it), packed back to back:
 *   packed  dev int32, 16-byte aligned: a 4-word header {valid records in all shards, fullest shard's count
 *           (> shard_capacity: records were dropped -- grow and scan again), records present behind the header
 *           = min(valid, packed_capacity), shard_capacity}, then that many WbDet records (shard order)
 * One contiguous prefix for a single host read-back (Model.detect, model.py:173-179) or one collective
 * (multi-GPU gather of detections); no host synchronisation. */
int wb_det_pack_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                       int32_t *packed, uint32_t packed_capacity);

/* Model.detect's last step in one launch (model.py:136-147, :173-179): for the valid records of all shards, at their
 * packed positions i < out_capacity,
 *   out  dev, 16-byte aligned:  int32 header[4] as wb_det_pack_launch writes it
 *                             | uint64 keys[out_capacity]   level << 54 | r << 40 | c << 26 | i
 *                             | float  boxes[out_capacity][4]   (c, r, c + n, r + m) * inv_scale[level]
 *                             | float  scores[out_capacity]
 * Sorting the keys gives the reference order (level, r, c); a sorted key's low 26 bits index boxes / scores.
 *   inv_scale  dev float32[n_levels] = float32(1 / scale) per level; m, n = window rows, cols
 *   n_levels, max_rows, max_cols  the scan's extent, checked against the key's 10 / 14 / 14 bits
 *   out_capacity  even, <= 2^26.   WB_ERR_UNSUPPORTED when the extent does not fit the key (use wb_det_pack_launch +
 *   wb_boxes_launch then).  No host synchronisation. */
int wb_det_finish_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                         const float *inv_scale, int n_levels, int max_rows, int max_cols, int m, int n,
                         void *out, uint32_t out_capacity);

/* wb_det_finish_launch with the ordering done on the device too (model.py:173-179: the concatenated result is in level
 * order, row-major inside a level): same arguments, same buffer layout, but when the valid records number at most
 * min(out_capacity, 4096) the three sections are written IN KEY ORDER -- keys[i] ascending, boxes[i] / scores[i] the
 * i-th detection of the reference's order (a key's low 26 bits then name the packed position the record came from and
 * carry no meaning for the caller) -- and header[3] = 1.  Otherwise header[3] = 0 and the sections are exactly what
 * wb_det_finish_launch writes (sort the keys, gather).  header[0..2] as wb_det_pack_launch writes them.
 *   tail, tail_words  optional (NULL, 0): dev int32 words copied behind the scores section, out + 16 + 28 * out_capacity
 *                     bytes -- the scan's alive[] statistics (model.py:248,252), so that ONE read-back carries all a
 *                     Model.detect call returns
 * No host synchronisation. */
int wb_det_finish_sorted_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                                const float *inv_scale, int n_levels, int max_rows, int max_cols, int m, int n,
                                void *out, uint32_t out_capacity, const int32_t *tail, uint32_t tail_words);

/* The same for a BATCH (the reference's detection loop over files, scripts/waldboost-detect.py:64-67, taken a batch at a
 * time): the shards' records are first split by image into buckets (scratch), then every image's bucket is ordered and
 * finished like a single image's shards.  Two launches, no host synchronisation.
 *   scratch  dev, 16-byte aligned, >= n_images * (256 + 16 * out_capacity) bytes
 *   out      dev, 16-byte aligned:  int32 info[4] = (valid records of all shards, fullest shard -- above
 *            shard_capacity: records were dropped, scan again --, n_images, out_capacity)
 *            | per image b, 16 + 28 * out_capacity bytes: header[4] | keys | boxes | scores exactly as
 *              wb_det_finish_sorted_launch writes them for ONE image with capacity out_capacity: header[0] = the image's
 *              detections, header[1] the same (above out_capacity: they did not fit), header[3] = 1 when in key order
 *   out_capacity  per image; a multiple of 4, <= 2^26 (ordered up to 4096 detections per image) */
int wb_det_order_batch_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                              int n_images, const float *inv_scale, int n_levels, int max_rows, int max_cols, int m, int n,
                              void *scratch, size_t scratch_bytes, void *out, uint32_t out_capacity);

/* One tree evaluated at explicit window origins (rs[i], cs[i]) of an HWC channel image
 * X[u][v][C] of x_dtype (WB_DTYPE_F32 / WB_DTYPE_U8); out[i] = prediction of the leaf reached
 * (training.py:84-96). Tree arrays and rs/cs/out are dev pointers. */
int wb_tree_eval_launch(void *stream, const void *X, int x_dtype, int u, int v, int C, const int32_t *rs,
                        const int32_t *cs, int64_t n_pos, const uint8_t *feature,
                        const float *threshold, const int8_t *left, const int8_t *right,
                        const float *prediction, int n_nodes, float *out);

/* Crops of m x n windows of an HWC channel image X[u][v][C] (x_dtype: WB_DTYPE_F32 / WB_DTYPE_U8) at the
 * origins (rs[i], cs[i]) -> out[n_pos][m][n][C] of the same dtype (reference samples.py:14-43
 * gather_samples, the crop step of hard-negative mining).  Origins must satisfy rs+m <= u, cs+n <= v
 * (the host wrapper checks).  All pointers dev. */
int wb_gather_samples_launch(void *stream, const void *X, int x_dtype, int u, int v, int C, const int32_t *rs,
                             const int32_t *cs, int64_t n_pos, int m, int n, void *out);

/* The cascade on per-sample arrays X[n_samples][m][n][C] (reference model.py:181-214 Model.predict, the
 * re-scoring step of the training sample pool): H[i] = accumulated response in stage order while the
 * sample is alive, -inf once a stage rejected it; mask[i] (uint8) = 1 if it passed every stage. */
int wb_samples_predict_launch(void *stream, const WbModel *model, const void *X, int x_dtype,
                              int64_t n_samples, float *H, uint8_t *mask);

/* Threshold calibration (direct backward pruning, Zhang & Viola 2007; the reference has no counterpart: its thetas come
 * from training.py fit_rejection_threshold while a stage is trained).  New symbols of ABI 8 (the version number did not
 * change: nothing that existed did).
 *
 * The stage-score trace of the cascade on per-sample arrays X[n_samples][m][n][C] (as wb_samples_predict_launch):
 *   trace  dev float32 [T][n_samples], STAGE-major (a wave's 64 samples store 256 contiguous bytes per stage), or NULL:
 *          trace[t][i] = running score of sample i after stage t: h = h + pred in fp32, in stage order, from 0.f
 *   final  dev float32 [n_samples] or NULL: the last row of the trace
 *   alive  dev uint32 [T + 1] or NULL: alive[t] = samples entering stage t (alive[0] = n_samples), alive[T] = samples
 *          that passed every stage; set inside the call, whatever it held
 *   reject 0: the thetas are ignored, every sample walks all T stages;  1: they apply as in the cascade (`h >= theta`,
 *          -inf never rejects): from the rejecting stage on a sample's trace entries and its final are -inf, so final is
 *          wb_samples_predict_launch's H.
 * Any output may be NULL, not all three (WB_ERR_INVALID).  n_samples == 0 succeeds without a launch. */
int wb_samples_trace_launch(void *stream, const WbModel *model, const void *X, int x_dtype, int64_t n_samples,
                            int reject, float *trace, float *final, uint32_t *alive);

/* The pruning step on the same samples: a sample is RETAINED when its unrejected final score is >= floor;
 *   stage_min   dev float32 [T]: the minimum over the retained samples of the unrejected running score after stage t
 *               (+inf everywhere when no sample is retained)
 *   n_retained  dev uint32 [1]: the number of retained samples
 * The walk is computed again (no N x T trace is read); the minimum is taken on order-preserving integer keys of the
 * floats, so it is exact and does not depend on order or run.  Both outputs are initialised inside the call (two memsets
 * on the stream).  n_samples == 0: +inf and 0. */
int wb_calib_min_launch(void *stream, const WbModel *model, const void *X, int x_dtype, int64_t n_samples,
                        float floor, float *stage_min, uint32_t *n_retained);

/* One tree on per-sample arrays X[n_samples][m][n][C]: node[i] = index of the leaf reached (reference
 * training.py:73-83 DTree.apply; DTree.predict is prediction[node]).  Tree arrays dev, as for
 * wb_tree_eval_launch. */
int wb_tree_apply_launch(void *stream, const void *X, int x_dtype, int64_t n_samples, int m, int n, int C,
                         const uint8_t *feature, const float *threshold, const int8_t *left,
                         const int8_t *right, int n_nodes, int32_t *node);

/* XYXY float32 boxes of detections: [c, r, c+n, r+m] * (1/scale[level]) (model.py:136-147).
 *   inv_scale  dev float[n_levels] = float32(1.0/scale) computed on the host in fp64 */
int wb_boxes_launch(void *stream, const WbDet *det, int64_t n_det, const float *inv_scale,
                    int m, int n, float *boxes /* [n_det][4] */, float *scores /* [n_det] */);

/* Greedy non-maximum suppression (reference testing.py:46 bbx.non_max_suppression; scripts/waldboost-detect.py:36).
 * New symbols of ABI 8 (the version number did not change: nothing that existed did).
 *   * when use_score_threshold != 0, boxes with `not (score >= score_threshold)` are dropped first;
 *   * the boxes are visited by score, highest first; -0.0 and +0.0 are equal; boxes of equal score in INPUT ORDER
 *     (NumPy: np.argsort(-scores, kind="stable")).  Scores must not be NaN;
 *   * a box is kept unless an already kept box of the same group has iou > iou_threshold with it (strict; a double);
 *   * iou in float64 on the float32 coordinates: iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih alike, inter = iw * ih,
 *     areas (x2 - x1) * (y2 - y1), union = area_a + area_b - inter, inter / union, 0 where union <= 0 -- every operation
 *     rounded on its own, the divide correctly rounded;
 *   * keep[i] = 1 for a kept box, 0 otherwise, in input order; n_keep[0] = their number.
 *   boxes    dev float32 [n][4] XYXY, 16-byte aligned;  scores dev float32 [n];  group dev int32 [n] or NULL (one group)
 *   scratch  dev, 16-byte aligned, wb_nms_scratch_bytes(n) bytes: per box 25 bytes (box, group, input index and dropped
 *            flag in visiting order), 16 bytes per 64 boxes (two bitmaps), 16 bytes of counters, rounded up to 256, then the
 *            suppression matrix of one BAND of rows: rows x ceil(n / 64) 64-bit words (upper triangle used).  A band is
 *            min(4096, n rounded up to 64) rows -- less, in multiples of 64, when that exceeds 64 MiB or when the caller
 *            hands in less: any size of at least the fixed part + 64 rows works, more bands are more launches.
 *   keep     dev uint8 [n];  n_keep dev uint32 [1]
 * wb_nms_launch finds the visiting order itself, by counting for every box the boxes in front of it: n * n comparisons,
 * 0.22 ms measured at 3 000 boxes (12 workgroups, each thread walking all boxes); a thread's walk grows with n, so some
 * 5 ms are to be expected at its limit of 2^16 boxes (WB_ERR_UNSUPPORTED above).
 * wb_nms_ordered_launch takes the visiting order from the caller: order dev uint32 [n], a permutation of 0 .. n - 1 -- the
 * stable descending sort of the scores (an entry >= n is skipped: that position visits nothing); n up to 2^26, what a
 * finish buffer's key can count.  What remains is the greedy algorithm's own cost: n * n / 2 float64 IoU tests (27 us at
 * 3 000 boxes) in bands of at most 4096 rows, three launches per band, the scan of a band on ONE wave (0.25 ms at 3 000
 * boxes, 1 700 of them kept).  10^5 boxes are 25 bands; 2^20 boxes are 5 * 10^11 tests in 2 048 bands of 512 rows (a
 * row is 128 KiB there) -- seconds, by that arithmetic, not by measurement; sizes beyond that are accepted for completeness, not because they are quick, and want
 * 8 * 64 * ceil(n / 64) bytes of matrix at the least.  wb_nms_scratch_bytes answers for both (n up to 2^26).
 * Three launches up to 4096 boxes.  No host synchronisation. */
int wb_nms_scratch_bytes(int64_t n, size_t *bytes);
int wb_nms_launch(void *stream, const float *boxes, const float *scores, const int32_t *group, int64_t n,
                  double iou_threshold, int use_score_threshold, float score_threshold, void *scratch,
                  size_t scratch_bytes, uint8_t *keep, uint32_t *n_keep);
int wb_nms_ordered_launch(void *stream, const float *boxes, const float *scores, const int32_t *group, const uint32_t *order,
                          int64_t n, double iou_threshold, int use_score_threshold, float score_threshold, void *scratch,
                          size_t scratch_bytes, uint8_t *keep, uint32_t *n_keep);

/* The same on a finish buffer, right behind the launch that wrote it and before the read-back:
 *   fin      dev: one image's block header[4] | keys | boxes | scores of capacity out_capacity as
 *            wb_det_finish_sorted_launch / wb_det_finish_launch wrote it; n_images > 1: image b's block at
 *            fin + b * (16 + 28 * out_capacity) bytes (wb_det_order_batch_launch's `out + 16`).  Not modified.
 *            header[3] == 1: the sections are in key order and the input order is the position; header[3] == 0: packed
 *            order, the input order is the KEY order (ties between equal scores go to the smaller key; equal keys, which
 *            no launch of this library writes, to the smaller position).  (The header[3]
 *            of wb_det_finish_launch is the shard capacity: for such a buffer the caller stores 0 there first.)
 *   result   dev, 4-byte aligned: per image 16 + out_capacity bytes:  uint32 info[4] = (kept boxes, boxes NMS ran over,
 *            done, 0) | uint8 keep[out_capacity], keep[i] for the box at position i of the sections.  done = 0: the image
 *            has more detections than the block holds or than 4096 -- nothing else was written for it (use
 *            wb_nms_launch on the complete result then).
 *   scratch  dev, 16-byte aligned, wb_nms_finish_scratch_bytes(out_capacity, n_images) bytes
 * out_capacity a multiple of 4.  One group.  Three launches for all images, no host synchronisation. */
int wb_nms_finish_scratch_bytes(uint32_t out_capacity, int n_images, size_t *bytes);
int wb_nms_finish_launch(void *stream, const void *fin, uint32_t out_capacity, int n_images, double iou_threshold,
                         int use_score_threshold, float score_threshold, void *scratch, size_t scratch_bytes,
                         void *result);

/* Box matching: for every detection the best IoU over the ground-truth boxes of its image and the box that gives it (reference
 * testing.py:53-58, the iou.argmax / iou.max of Evaluator.evaluate; samples.py:133 for the miner).
 * New symbol of ABI 8 (the version number did not change: nothing that existed did).
 *   dt        dev float64 [n_dt][4] XYXY, 8-byte aligned;  dt_image dev int32 [n_dt]: the image each detection belongs to
 *   gt        dev float64 [n_gt][4] XYXY, 8-byte aligned (NULL allowed when n_gt == 0);  gt_off dev int32 [n_images + 1]: the
 *             candidates of image b are gt[gt_off[b] .. gt_off[b + 1])
 *   best      dev float64 [n_dt], 8-byte aligned;  owner dev int32 [n_dt]
 *   * iou in float64: iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih alike, inter = iw * ih, areas (x2 - x1) * (y2 - y1),
 *     union = area_a + area_b - inter, inter / union, 0 where union <= 0 -- every operation rounded on its own, the divide
 *     correctly rounded (waldboost_amd.boxes.iou, operation by operation);
 *   * best[i] = the largest iou over the candidates of detection i; owner[i] = the FIRST candidate that reaches it, as an index
 *     inside the image's own list (np.argmax: a detection that overlaps nothing is owned by candidate 0);
 *   * an image without candidates: best 0, owner -1.
 * Every entry of best and owner is written.  dt_image is clamped to [0, n_images) and both ends of a candidate range to
 * [0, n_gt] (an end in front of its start: no candidates), so bad offsets read nothing outside the buffers.
 * n_dt == 0 launches nothing (WB_OK, pointers not looked at); n_dt > 2^26 is WB_ERR_UNSUPPORTED; null pointers, negative
 * sizes, n_images == 0 with detections and misaligned pointers are WB_ERR_INVALID.  One launch, no scratch, no host
 * synchronisation. */
int wb_match_launch(void *stream, const double *dt /* [n_dt][4] */, const int32_t *dt_image /* [n_dt] */,
                    const double *gt /* [n_gt][4] */, const int32_t *gt_off /* [n_images + 1] */,
                    int64_t n_dt, int64_t n_gt, int n_images, double *best /* [n_dt] */, int32_t *owner /* [n_dt] */);

/* Box voting: every box that non-maximum suppression kept becomes the weighted mean of the boxes of its cluster, and the
 * cluster is counted (Viola-Jones's merge of overlapping detections; OpenCV's minNeighbors).  DESIGN.md 4.16 has the rule,
 * tests/vote_reference.py states it in NumPy.  New symbol of ABI 8 (the version number did not change: nothing that existed did).
 *   boxes    dev float32 [n][4] XYXY, 16-byte aligned;  scores dev float32 [n], no NaN;  group dev int32 [n] or NULL (one group)
 *   keep     dev uint8 [n] as wb_nms_launch wrote it (any non-zero byte: kept)
 *   merged   dev float32 [n][4], 16-byte aligned, not overlapping boxes;  votes dev int32 [n]
 *   * a box is LIVE unless use_score_threshold != 0 and `not (score >= score_threshold)` -- the boxes NMS dropped first;
 *   * for a kept box k, box j is a VOTER when j == k (always, even for a box of no area, whose iou with itself is 0), or when
 *     j is live, group[j] == group[k] and iou(box_k, box_j) >= vote_iou (a double);
 *   * iou exactly as for wb_nms_launch / wb_match_launch: float64 on the float32 coordinates, every operation rounded on
 *     its own, the divide correctly rounded;
 *   * weights WB_VOTE_UNIFORM: w_j = 1.0;  WB_VOTE_SCORE: w_j = float64(score_j) - float64(score_threshold), >= 0 for every
 *     live box; the mode needs use_score_threshold, and a box that is not live never votes except for itself;
 *   * the order of the sums is fixed and part of the contract (it does not depend on the launch geometry, on chunking or on
 *     the run): lane l of 64 visits the candidates j = l, l + 64, l + 128, ... ascending and for each voter computes
 *     sw = sw + w and, for each of the four coordinates, sc[i] = sc[i] + (w * float64(x_ji)) -- the product rounded first,
 *     then the sum, no fused multiply-add; the 64 partials of each of the five doubles and of the integer vote count are
 *     combined by a butterfly: for s = 1, 2, 4, 8, 16, 32: p = p + p[lane ^ s];
 *   * merged[k][i] = float32(sc[i] / sw) when sw > 0 (the divide correctly rounded, the cast round-to-nearest-even); when sw
 *     is not > 0 (every voter exactly at the threshold) box k's own coordinates;  votes[k] = the number of voters, >= 1;
 *   * the row of a box that is not kept holds its own box and votes = 0.  Every row is written.
 * Cost: K * n float64 IoU tests, K the number of kept boxes.  One wave per box, candidates staged through LDS 256 at a time
 * and shared by a workgroup's four waves.
 * n == 0 launches nothing (WB_OK, pointers not looked at); n > 2^26 is WB_ERR_UNSUPPORTED; null pointers (group may be
 * NULL), misaligned pointers, a negative n, a NaN or negative vote_iou, a NaN score_threshold in use, an unknown weights
 * code and WB_VOTE_SCORE without a threshold are WB_ERR_INVALID, refused before any HIP call.  One launch, no atomics, no
 * scratch, no host synchronisation. */
#define WB_VOTE_UNIFORM 0
#define WB_VOTE_SCORE 1
int wb_vote_launch(void *stream, const float *boxes, const float *scores, const int32_t *group,
                   const uint8_t *keep, int64_t n, double vote_iou, int weights,
                   int use_score_threshold, float score_threshold,
                   float *merged, int32_t *votes);

/* Hard-negative mining of a scanned batch: label, choose and crop on the device (reference samples.py:46-216 label_boxes,
 * select_candidates, gather_samples; DESIGN.md 4.12 has the rule, tests/mine_reference.py states it in NumPy).
 * New symbols of ABI 8 (the version number did not change: nothing that existed did).
 * wb_mine_select_launch:
 *   det        dev WbDet [n_det], 16-byte aligned, ANY order (e.g. wb_det_pack_launch's records); image and level are clamped
 *              into [0, n_images) and [0, n_levels); (image, level, r, c) must be unique (a scan's records are)
 *   inv_scale  dev float [n_levels] as for wb_boxes_launch: the box of a record is float32 [c, r, c+n, r+m] * inv_scale[level]
 *   gt, gt_off as for wb_match_launch (both ends of a range clamped to [0, n_gt]);  gt_ignore dev uint8 [n_gt];
 *   serial     dev uint32 [n_images]: the caller's number of each image (what its keys depend on instead of its batch slot)
 *   * best / owner of a record: wb_match_launch's, on the float32 box;
 *   * FP hit: best < max_fp_iou, or an image without candidates;  TP hit: candidates, best > min_tp_iou (both strict, float64)
 *     and gt_ignore[owner] == 0;  want_tp / want_fp == 0: that class has no hits;
 *   * key = fmix32(((r << 16) | c) ^ g), g = fmix32(fmix32(seed ^ fmix32(serial[image] + 0x9E3779B9)) ^ (level * 0x9E3779B1)),
 *     fmix32(x): x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13, x *= 0xC2B2AE35, x ^= x >> 16 (uint32);
 *   * per (image, level) and class, of H hits the min(H, max_tp) / min(H, max_fp) with the smallest keys are chosen;
 *     label 1 (TP) or -1 (FP); a record chosen for both is FP.
 *   rows       dev, 16-byte aligned: the chosen records as 32-byte rows {WbDet det; double best; int32 owner; int32 label},
 *              in NO particular order (the caller orders them by (image, level, r, c)); n_rows dev uint32 [1]: their number.
 *              out_capacity rows of room: at least min(n_det, n_images * n_levels * (max_tp + max_fp)) (caps of classes
 *              that are not wanted count as 0), which the rule cannot exceed -- less is WB_ERR_INVALID
 *   scratch    dev, 16-byte aligned, wb_mine_scratch_bytes(n_det, n_images, n_levels) bytes (6 per record, 2 KiB + 32 per
 *              group); its content on entry does not matter
 * n_det == 0 launches nothing (WB_OK, n_rows untouched).  Null or misaligned pointers, a short scratch, negative sizes or caps,
 * records of no image or level: WB_ERR_INVALID.  More than 2^26 records, 1024 images, 256 levels or 16384 (image, level)
 * groups: WB_ERR_UNSUPPORTED.  One memset and nine launches (an 8-bit digit select: no sort, no host synchronisation).
 * wb_mine_gather_launch: out[i][m][n][C] = the window of rows[i] in the pyramid buffer `buf` (dtype WB_DTYPE_F32 / WB_DTYPE_U8):
 *   level l of image b is HWC [u][v][C] at buf + b * img_stride + levels[l].chn_off (elements).  A row whose image or level is
 *   out of range, whose window leaves its level (r + m > u or c + n > v) or whose level leaves the image's stride is written
 *   as zeros and sets err[0] = 1 (err dev uint32 [1], 0 otherwise): nothing outside n_images * img_stride elements is read.
 *   One memset and one launch, no host synchronisation. */
typedef struct WbMineLevel {
    int64_t chn_off;
    int32_t u, v;
} WbMineLevel; /* 16 bytes */
int wb_mine_scratch_bytes(int64_t n_det, int n_images, int n_levels, size_t *bytes);
int wb_mine_select_launch(void *stream, const WbDet *det, int64_t n_det, const float *inv_scale, int n_levels, int m, int n,
                          const double *gt, const int32_t *gt_off, const uint8_t *gt_ignore, int64_t n_gt, const uint32_t *serial,
                          int n_images, double min_tp_iou, double max_fp_iou, int64_t max_tp, int64_t max_fp, int want_tp,
                          int want_fp, uint32_t seed, void *scratch, size_t scratch_bytes, void *rows, int64_t out_capacity,
                          uint32_t *n_rows);
int wb_mine_gather_launch(void *stream, const void *buf, int dtype, int64_t img_stride, int n_images, const WbMineLevel *levels,
                          int n_levels, int C, const void *rows, int64_t n_rows, int m, int n, void *out, uint32_t *err);

/* Multiple-instance pruning of a finished cascade (Zhang & Viola 2007; the reference has no counterpart; DESIGN.md 4.14 has the
 * rule, tests/mip_reference.py states it in NumPy).  New symbols of ABI 8 (the version number did not change: nothing that
 * existed did).
 * wb_mip_windows_launch: the acceptable windows of the window grids of n_images pyramids against their ground truth.
 *   levels_host     HOST WbMineLevel [n_levels]: level l is u x v channels (chn_off is not looked at: no pyramid is read); its
 *                   windows are those the scan visits, r in [0, u - m), c in [0, v - n); u, v in [0, 65536]
 *   inv_scale_host  HOST float [n_levels], wb_boxes_launch's values: the box of a window is float32 [c, r, c+n, r+m] * inv_scale[l]
 *   gt, gt_off, gt_ignore  as for wb_mine_select_launch (dev; both ends of a range clamped to [0, n_gt])
 *   * best / owner of a window: wb_match_launch's (float64 IoU, operation by operation; the FIRST candidate that reaches the
 *     maximum);
 *   * a window is ACCEPTABLE when its image has candidates, best > min_iou (strict, float64) and gt_ignore[owner] == 0 --
 *     wb_mine_select_launch's TP hit, without caps; it belongs to the bag of its owner only.
 *   rows       dev, 16-byte aligned: the acceptable windows as wb_mine_select_launch's 32-byte rows {WbDet det (score 0); double
 *              best; int32 owner; int32 label = 1}, in NO particular order.  n_rows dev uint32 [1]: their FULL number, also when
 *              it exceeds out_capacity: rows beyond the capacity are not written, the caller allocates n_rows rows and calls again.
 * One thread per window; an image's ground truth passes through LDS in chunks of 256 boxes.  One memset and one launch per
 * level that has windows; no scratch, no host synchronisation.  No window or n_gt == 0: n_rows = 0 without a launch.
 * Negative sizes, null or misaligned pointers, a level beyond 65536: WB_ERR_INVALID.  More than 1024 images, 256 levels,
 * 16384 (image, level) groups or 2^32 - 1 windows: WB_ERR_UNSUPPORTED.
 * wb_mip_prune_launch: the stage-sequential prune over bags.
 *   trace      dev float32 [n_stages][stride], stride >= n_windows: the unrejected running scores of the acceptable windows
 *              (wb_samples_trace_launch with reject = 0); no NaN
 *   bag        dev int32 [n_windows]: the bag of every window; a window whose bag lies outside [0, n_bags) is never retained;
 *              bag ids without windows are legal and contribute nothing
 *   * a window is retained at the start when trace[n_stages - 1][i] >= floor;
 *   * for t = 0 .. n_stages - 1, in order: theta[t] = the minimum, over the bags that have a retained window, of the maximum of
 *     trace[t][i] over the bag's retained windows; then every retained window with `not (trace[t][i] >= theta[t])` (the
 *     cascade's test) stops being retained: removed_at[i] = t;
 *   * maxima and minima are taken on the order-preserving integer keys of the floats (as wb_calib_min_launch: -0 below +0), so
 *     they are exact and depend neither on the order of the windows nor on the run.
 *   theta      dev float32 [n_stages]: +inf everywhere when no window is retained
 *   removed_at dev int32 [n_windows]: -1 for a window never retained, n_stages for one that survives every stage
 *   counts     dev uint32 [2]: the bags with a window retained at the start; the windows that survive every stage
 *   scratch    dev, 4-byte aligned, wb_mip_scratch_bytes(n_bags) bytes (4 per bag); its content on entry does not matter,
 *              nor does that of the outputs
 * Every retained bag keeps a window through all stages (the one that holds the bag's maximum at a stage is at or above that
 * stage's theta).  A stage depends on the one before it through one number; the dependency is carried by the order of
 * 2 * n_stages + 3 small launches (and three memsets) enqueued back to back: no workgroup waits for another and there is
 * no host synchronisation.  n_windows == 0, n_stages == 0 or n_bags == 0: +inf, -1 and zeros by memsets alone.
 * Negative sizes, stride < n_windows, (n_stages - 1) * stride + n_windows >= 2^31, n_bags >= 2^31, null or misaligned
 * pointers, a short scratch: WB_ERR_INVALID. */
int wb_mip_windows_launch(void *stream, const WbMineLevel *levels_host, const float *inv_scale_host, int n_levels, int m, int n,
                          const double *gt, const int32_t *gt_off, const uint8_t *gt_ignore, int64_t n_gt, int n_images,
                          double min_iou, void *rows, int64_t out_capacity, uint32_t *n_rows);
int wb_mip_scratch_bytes(int64_t n_bags, size_t *bytes);
int wb_mip_prune_launch(void *stream, const float *trace, int64_t stride, int n_stages, int64_t n_windows, const int32_t *bag,
                        int64_t n_bags, float floor, void *scratch, size_t scratch_bytes, float *theta, int32_t *removed_at,
                        uint32_t *counts);

/* Split search of the FPGA flavour's tree learner (reference fpga/training.py:15-57), one tree level per call.
 * New symbols of ABI 8 (the version number did not change: nothing that existed did).
 *   xt       dev uint8 [n_features][n_samples]: the samples, FEATURE-major
 *   q        dev uint64 [n_samples], 8-byte aligned: the split weights as integers, rint(w' * 2^62), w' the weights with
 *            each class divided by twice its sum (fpga/training.py:105-107) -- every sum is an integer add, so results do
 *            not depend on the order of samples or on the run; a sum converts back as double(sum) * 2^-62
 *   cls      dev uint8 [n_samples]: 0 / 1
 *   node     dev int32 [n_samples]: the tree node (breadth-first id) each sample sits in
 *   level_base, n_level, slot: the level's nodes have ids level_base .. level_base + n_level - 1 (n_level <= 8); slot is a
 *            HOST array int8 [n_level]: the open slot 0 .. n_open - 1 of each, -1 for a leaf.  Samples of other nodes and
 *            of leaves take no part.  An open node must hold at least one sample.
 *   allowed  dev int32 [n_allowed]: the ordered feature list A (every entry in 0 .. n_features - 1)
 *   scratch  dev, 16-byte aligned, wb_fit_scratch_bytes(n_allowed, n_open) bytes: one (float64 metric, int32 t) record per
 *            (open node, entry of A) and two float64 totals per open node
 *   splits   dev WbFitSplit [n_open], 8-byte aligned: per open slot the first entry of A with the largest metric and its
 *            smallest best threshold t (candidates xmin .. xmax + 1 over the node's samples: 256 is a legal value), the
 *            metric, and the node's class totals T0, T1.  A NaN metric is the largest (np.argmax): a node without weight
 *            in one class answers (A[0], its xmin).
 * Two launches (histograms and per-feature argmax: one workgroup per entry of A, (4 + 1) KiB of LDS per open node; then
 * the argmax over A), no host synchronisation.
 * wb_fit_route_launch applies the splits (fpga/training.py:133-138): a sample of open slot s moves to node
 * child_base + 2 * s when x[feature] <= t, to child_base + 2 * s + 1 otherwise (breadth-first numbering: the children of
 * a level's open nodes follow each other in slot order).  node is updated in place. */
#define WB_FIT_MAX_OPEN 8
typedef struct {
    int32_t feature;    /* flat index into the (m, n, C) sample */
    int32_t threshold;  /* t: the node routes with x <= t (the metric rated x < t -- the reference's own difference) */
    double metric, t0, t1;
} WbFitSplit;           /* 32 bytes */
int wb_fit_scratch_bytes(int n_allowed, int n_open, size_t *bytes);
int wb_fit_level_launch(void *stream, const uint8_t *xt, int64_t n_samples, int64_t n_features, const uint64_t *q,
                        const uint8_t *cls, const int32_t *node, int level_base, int n_level, const int8_t *slot,
                        int n_open, const int32_t *allowed, int n_allowed, void *scratch, size_t scratch_bytes,
                        WbFitSplit *splits);
int wb_fit_route_launch(void *stream, const uint8_t *xt, int64_t n_samples, int64_t n_features, int32_t *node,
                        int level_base, int n_level, const int8_t *slot, int n_open, const WbFitSplit *splits,
                        int child_base);

/* Split search of the base tree learner on float32 samples (reference training.py:33-50: scikit-learn's
 * DecisionTreeClassifier(class_weight="balanced"), gini, best splitter).  New symbols of ABI 8 (the version number did not
 * change: nothing that existed did).  The exact rules are stated at the head of csrc/wb_cart.hip.
 *
 * wb_cart_sort_launch, once per fit:
 *   xt       dev float32 [n_features][n_samples]: the samples, FEATURE-major; finite values
 *   order    dev int32 [n_features][n_samples], written: per feature the sample indices sorted by (value, index), -0.0
 *            equal to +0.0
 * n_samples <= WB_CART_MAX_SAMPLES, n_features <= WB_CART_MAX_FEATURES (WB_ERR_UNSUPPORTED beyond).  One workgroup per
 * column, 32 KiB of LDS.
 *
 * wb_cart_level_launch, once per tree level: four launches (scan, best, move, part), no host synchronisation.
 *   q        dev uint64 [n_samples], 8-byte aligned: the split weights as integers; a sum converts back as
 *            double(sum) * scale, scale a power of two
 *   cls      dev uint8 [n_samples]: 0 / 1
 *   order_in dev int32 [n_features][n_samples]: every column sorted and partitioned by node: the level's open node k is
 *            positions begin[k] .. end[k] - 1 of EVERY column (the root: 0 .. n_samples - 1 of wb_cart_sort_launch's output)
 *   order_out dev, like order_in and not the same buffer, written: for every open node that was split, its segment with
 *            the left child's samples first (begin[k] .. begin[k] + n_left - 1), then the right child's, each still sorted.
 *            Other positions are not written.
 *   node     dev int32 [n_samples], updated: a sample of a split open node k gets child_base + 2 * k (left) or
 *            child_base + 2 * k + 1 (right); other entries stay
 *   begin, end, t0, t1   HOST arrays [n_open]: the segments (ascending, disjoint, non-empty) and the nodes' integer class
 *            totals (each below 2^62)
 *   scratch  dev, 16-byte aligned, wb_cart_scratch_bytes(n_features, n_open) bytes
 *   splits   dev WbCartSplit [n_open], 8-byte aligned: per open node the winning candidate, feature = -1 when no feature
 *            has one (the node is a leaf and nothing of it moves).  The node routes with
 *            double(x[feature]) <= lo / 2.0 + hi / 2.0 (lo when that sum equals hi or is infinite). */
#define WB_CART_MAX_SAMPLES 65536
#define WB_CART_MAX_FEATURES 65536
typedef struct {
    int32_t feature;    /* flat index into the (m, n, C) sample, -1: no candidate */
    int32_t n_left;     /* p: the number of samples that go left */
    float lo, hi;       /* xs[p - 1], xs[p] of the node's samples sorted by the feature */
    double proxy;       /* -inf when there is no candidate */
    double t0, t1;      /* the node's class totals, double(T) * scale */
} WbCartSplit;          /* 40 bytes */
int wb_cart_sort_launch(void *stream, const float *xt, int64_t n_samples, int64_t n_features, int32_t *order);
int wb_cart_scratch_bytes(int64_t n_features, int n_open, size_t *bytes);
int wb_cart_level_launch(void *stream, const float *xt, int64_t n_samples, int64_t n_features, const uint64_t *q,
                         const uint8_t *cls, const int32_t *order_in, int32_t *order_out, int32_t *node, int n_open,
                         const int32_t *begin, const int32_t *end, const uint64_t *t0, const uint64_t *t1, double scale,
                         int min_samples_leaf, int child_base, void *scratch, size_t scratch_bytes, WbCartSplit *splits);

/* CNN re-scoring of detection windows: out[i] = cnn(X[i]) + scores_in[i], the forward pass of the reference's
 * verification.model_cnn (reference verification.py:28-56) for a window shape (m, n, C).  New symbols of ABI 8 (the version
 * number did not change: nothing that existed did).  The arithmetic contract is stated at the head of csrc/wb_verify.hip:
 * every pre-activation one float32 fmaf chain in a fixed order, so a window's result depends on nothing but the window.
 *
 * Supported: 2 <= m, n <= 32, 1 <= C <= 16 (WB_ERR_UNSUPPORTED otherwise, from all three entry points).
 * m2 = m / 2, n2 = n / 2, F = m2 * n2 * 16.
 *
 * The packed float32 weight buffer (wb_verify_weights_floats gives its length), batch normalisation already folded in
 * (W' = float32(W * s[o]), b' = float32((b - mean) * s + beta), s = gamma / sqrt(variance + epsilon), in float64):
 *   conv1  W' [3][3][C][8]   then b' [8]
 *   conv2  W' [3][3][8][8]   then b' [8]
 *   conv3  W' [3][3][8][16]  then b' [16]
 *   conv4  W' [3][3][16][16] then b' [16]
 *   dense0 kernel [F][128] (row = flat (row, column, channel) index of the pooled 16-channel map) then bias [128]
 *   dense1 kernel [128] then bias [1]
 * The convolution kernels keep Keras's (ky, kx, input channel, output channel) order; every value must be finite.
 *
 *   X          dev [n_windows][m][n][C], x_dtype WB_DTYPE_F32 (4-byte aligned) or WB_DTYPE_U8 (widened exactly)
 *   weights    dev float32, 16-byte aligned, the packed buffer
 *   scores_in  dev float32 [n_windows];  out dev float32 [n_windows]: every entry written, nothing behind them
 *   scratch    dev, 16-byte aligned, wb_verify_scratch_bytes(m, n, C, n_windows) bytes: the features [n_windows][F].
 *              Nothing in it needs clearing between calls.
 * n_windows == 0 launches nothing (WB_OK, pointers not looked at); more than 2^26 windows or another x_dtype is
 * WB_ERR_UNSUPPORTED; null pointers, misaligned pointers, a negative count and a short scratch are WB_ERR_INVALID.  Two
 * launches, no host synchronisation. */
int wb_verify_weights_floats(int m, int n, int C, int64_t *count);
int wb_verify_scratch_bytes(int m, int n, int C, int64_t n_windows, size_t *bytes);
int wb_verify_launch(void *stream, const void *X, int x_dtype, int64_t n_windows, int m, int n, int C, const float *weights,
                     const float *scores_in, void *scratch, size_t scratch_bytes, float *out);

/* Training of the verification CNN: one step of Keras's train_on_batch for model_cnn under the reference's exploss and
 * Adam (reference verification.py:59-81).  New symbols of ABI 8 (additive: the version number did not change).  The
 * step's contract -- batch statistics, loss, backward rules, the dropout generator, Adam, the fixed summation orders --
 * is stated at the head of csrc/wb_verify_train.hip and in tests/verify_train_reference.py.
 *
 * Supported: wb_verify_launch's window shapes, and an even batch of 2 .. 1024 windows (WB_ERR_UNSUPPORTED otherwise,
 * before any launch).
 *
 * The training layout (wb_verify_train_param_floats gives its length): the 28 arrays of model_cnn(...).get_weights()
 * in Keras's order, unfolded, float32, one after the other -- per convolution block kernel [3][3][Cin][Cout], bias,
 * gamma, beta, moving_mean, moving_variance; then the dense kernel [F][128], its bias, the dense kernel [128], its bias.
 * params, adam_m, adam_v and grads_out all have this layout.  Of adam_m / adam_v the slots of the convolution biases and
 * of the moving statistics are never touched.
 *
 *   X, H, Y    the resident sample pool: dev [n_pool][m][n][C] crops of x_dtype (WB_DTYPE_F32 / WB_DTYPE_U8, widened
 *              exactly), dev float32 [n_pool] detector scores and targets (-1 / +1)
 *   idx        dev int32 [batch]: the step's windows, as indices into the pool; duplicates are allowed and each counts.
 *              The caller keeps them inside 0 .. n_pool - 1 (the kernels clamp, so nothing outside the pool is read).
 *   params, adam_m, adam_v    dev float32, 16-byte aligned, updated in place
 *   t          dev int32 [2]: t[0] the number of steps done (0 before the first; the dropout masks and Adam's bias
 *              correction follow it), advanced by the update kernel; t[1] is the update kernel's workgroup counter: zero
 *              before the first step, and left zero by every step
 *   hyper      host: the step's constants (Keras's defaults: lr 1e-4, beta1 0.9, beta2 0.999, adam_epsilon 1e-7,
 *              momentum 0.99, bn_epsilon 1e-3; dropout 0.2).  An element is kept iff its 32 bits of the generator are
 *              >= round(dropout * 2^32); kept values are multiplied by float32(1 / (1 - dropout)).
 *   scratch    dev, 16-byte aligned, wb_verify_train_scratch_bytes(m, n, C, batch) bytes; nothing in it needs clearing
 *   loss_out   dev float32 [1]: the step's loss (before the update)
 *   grads_out  null, or dev float32 in the training layout: the step's gradients; the convolution biases' slots receive
 *              0 (their gradient is zero by contract), the moving_mean / moving_variance slots the step's batch mean and
 *              unbiased batch variance
 * Null or misaligned pointers, n_pool < 1, a short scratch and constants out of range are WB_ERR_INVALID.  A chain of
 * launches on `stream`, no host synchronisation; the same inputs give the same bits. */
typedef struct {
    double lr, beta1, beta2, adam_epsilon;
    double momentum, bn_epsilon;    /* batch normalisation: moving-average momentum, variance epsilon */
    double dropout;                 /* rate, 0 <= dropout < 1 */
    uint32_t seed;                  /* of the dropout generator */
    uint32_t reserved;              /* 0 */
} WbVerifyTrainHyper;               /* 64 bytes */
int wb_verify_train_param_floats(int m, int n, int C, int64_t *count);
int wb_verify_train_scratch_bytes(int m, int n, int C, int64_t batch, size_t *bytes);
int wb_verify_train_step(void *stream, const void *X, int x_dtype, const float *H, const float *Y, int64_t n_pool,
                         const int32_t *idx, int64_t batch, int m, int n, int C, float *params, float *adam_m, float *adam_v,
                         int32_t *t, const WbVerifyTrainHyper *hyper, void *scratch, size_t scratch_bytes, float *loss_out,
                         float *grads_out);

/* Box regression: a linear map from a window's channel values to four box offsets (the reference computes the target,
 * samples.py:152-157 get_regression_target, and never uses it).  DESIGN.md 4.15 has the rule, tests/regress_reference.py
 * states it in NumPy.  New symbols of ABI 8 (the version number did not change: nothing that existed did).
 *
 * wb_gram_launch: S += A^T A for A = [X | 1 | T], n_rows x P, P = D + 5, in float64 -- the streaming normal equations.
 *   X        dev [n_rows][D], x_dtype WB_DTYPE_U8 or WB_DTYPE_F32 (4-byte aligned), widened exactly
 *   T        dev double [n_rows][4];  S dev double [P][P], read and updated; symmetric on entry (its upper triangle is
 *            what is read; every entry is written)
 *   scratch  dev, 8-byte aligned, wb_gram_scratch_bytes(n_rows, D) bytes; its content on entry does not matter
 * The contraction runs on v_mfma_f64_16x16x4_f64, tile pairs ti <= tj only.  Determinism is part of the contract and there
 * are no floating-point atomics: rows are cut into chunks of WB_GRAM_CHUNK, whatever the grid; every (tile, chunk) partial
 * goes to scratch; a second launch adds a tile's partials in ascending chunk order, adds that sum to S and writes the
 * mirrored entry with the same bits.  So the result depends on the inputs and the sequence of calls alone, is bitwise
 * symmetric and the same from run to run.  Rows past n_rows count as zeros.  Inside a chunk the order of the adds is the
 * instruction's: a result lies within (n_rows + 8) * 2^-52 * (|A|^T |A|) of the exact one, and is exact while the
 * integers stay below 2^53.
 * n_rows == 0: WB_OK without a launch.  P > WB_GRAM_MAX_P, more than 2^26 rows or another x_dtype: WB_ERR_UNSUPPORTED.
 * Null or misaligned pointers, negative sizes, D < 1, a short scratch: WB_ERR_INVALID.  Two launches, no host synchronisation.
 *
 * wb_regress_predict_launch: pred[i][k] = sum_j X[i][j] * Wb[j][k] + Wb[D][k] on crops X [n][m][nn][C] (x_dtype as above),
 *   D = m * nn * C, feature j = (r * nn + c) * C + ch; Wb dev double [D + 1][4] (the last row is the intercept), pred dev
 *   double [n][4].  One wave per window, in a fixed order: lane l of 64 keeps four float64 partials from 0 and adds
 *   x[j] * Wb[j][k] for j = l, l + 64, ... ascending (product and sum rounded separately); then for s = 32, 16, 8, 4, 2, 1:
 *   p[l] = p[l] + p[l ^ s]; pred[k] = p[0][k] + Wb[D][k].
 * wb_regress_apply_launch: the same on windows read where they lie in the pyramid -- buf, dtype, img_stride, n_images,
 *   levels, n_levels, C and the error word exactly as for wb_mine_gather_launch; det dev WbDet [n_det], 16-byte aligned;
 *   inv_scale dev float [n_levels] as for wb_boxes_launch; inv64 dev double [n_levels] = 1.0 / scale, computed on the host.
 *   boxes dev float [n_det][4]: float32(float64(box) - pred * inv64[level]), box = float32 [c, r, c+nn, r+m] *
 *   inv_scale[level]; pred dev double [n_det][4] or NULL.  A record whose image or level is out of range, whose window
 *   leaves its level or whose level leaves the image's stride sets err[0] = 1 and gets its unrefined box (of the level
 *   clamped into range) and a zero pred: nothing outside n_images * img_stride elements is read.  No crop is materialised.
 * n == 0: nothing is launched (apply clears err).  More than 2^26 windows or another dtype: WB_ERR_UNSUPPORTED.  Null or
 * misaligned pointers and negative sizes: WB_ERR_INVALID.  One launch (apply: and one memset), no host synchronisation. */
#define WB_GRAM_CHUNK 256
#define WB_GRAM_MAX_P 2048
int wb_gram_scratch_bytes(int64_t n_rows, int D, size_t *bytes);
int wb_gram_launch(void *stream, const void *X, int x_dtype, const double *T, int64_t n_rows, int D, double *S, void *scratch,
                   size_t scratch_bytes);
int wb_regress_predict_launch(void *stream, const void *X, int x_dtype, int64_t n, int m, int nn, int C, const double *Wb,
                              double *pred);
int wb_regress_apply_launch(void *stream, const void *buf, int dtype, int64_t img_stride, int n_images, const WbMineLevel *levels,
                            int n_levels, int C, const WbDet *det, int64_t n_det, int m, int nn, const double *Wb,
                            const float *inv_scale, const double *inv64, double *pred, float *boxes, uint32_t *err);

/* Device self-test: the uint8 fast path of the orientation projection (fp32 arithmetic that is
 * proven equal to the reference's fp64 formula for integer gradients) is compared with the fp64
 * formula for every (gx, gy) in [-1020, 1020]^2; *mismatches (dev uint32, zeroed by the caller)
 * receives the number of differing channel values -- must stay 0. */
int wb_selftest_projection(void *stream, uint32_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif /* WALDBOOST_HIP_H */
