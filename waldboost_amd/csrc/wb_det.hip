// From the cascade's sharded detection records to results, on gfx950.
//
// Replaces reference model.py:136-147 (Model.get_boxes) and :173-179 (Model.detect's concatenated result: levels in pyramid
// order, windows row-major inside a level).  A scan leaves its records in WB_DET_SHARDS shards of `cap` records with one
// counter each (a counter above cap: records were dropped, scan again).  This file holds what reads them:
//   * boxes_kernel                  get_boxes of a record list (wb_boxes_launch);
//   * det_pack_kernel               the valid records back to back behind a 4-word header (wb_det_pack_launch);
//   * det_finish_kernel             sort keys, boxes and scores at the packed positions (wb_det_finish_launch);
//   * det_finish_sorted_kernel<16>  the same in the reference's order (wb_det_finish_sorted_launch);
//   * det_bucket_kernel + det_finish_sorted_kernel<4>   a batch's records by image, each image ordered
//                                   (wb_det_order_batch_launch).
// Every step the kernels share stands here once: the shard prefix, the sort key, the box arithmetic (wb_match_iou.h), the unordered finish
// of one shard and the bisection from a packed position to its record.  Each is a bit-exactness contract with the
// reference's get_boxes and result order.
#include "wb_match_iou.h"   // window_box: Model.get_boxes' arithmetic, shared with the labelling of windows

namespace {

static_assert(WB_DET_SHARDS == 64, "one shard counter per lane of a wave, one workgroup per shard");

// ---- the sort key: level | r | c | packed position.  Sorting these 64-bit words IS the reference order (level, r, c), and
//      the low bits say where the sorted record's box and score lie.  (readback.py decodes it on the host.)
constexpr int DET_KEY_LEVEL_BITS = 10, DET_KEY_ROW_BITS = 14, DET_KEY_COL_BITS = 14, DET_KEY_POS_BITS = 26;
constexpr int DET_KEY_COL_SHIFT = DET_KEY_POS_BITS, DET_KEY_ROW_SHIFT = DET_KEY_COL_SHIFT + DET_KEY_COL_BITS,
              DET_KEY_LEVEL_SHIFT = DET_KEY_ROW_SHIFT + DET_KEY_ROW_BITS;
static_assert(DET_KEY_LEVEL_SHIFT + DET_KEY_LEVEL_BITS == 64, "the four fields fill the word");

__device__ inline unsigned long long det_key(uint32_t level, uint32_t r, uint32_t c, uint32_t at) {
    return ((unsigned long long)level << DET_KEY_LEVEL_SHIFT) | ((unsigned long long)r << DET_KEY_ROW_SHIFT) |
           ((unsigned long long)c << DET_KEY_COL_SHIFT) | (unsigned long long)at;
}
__device__ inline uint32_t det_key_level(unsigned long long key) { return (uint32_t)(key >> DET_KEY_LEVEL_SHIFT); }
__device__ inline uint32_t det_key_row(unsigned long long key) { return (uint32_t)(key >> DET_KEY_ROW_SHIFT) & ((1u << DET_KEY_ROW_BITS) - 1u); }
__device__ inline uint32_t det_key_col(unsigned long long key) { return (uint32_t)(key >> DET_KEY_COL_SHIFT) & ((1u << DET_KEY_COL_BITS) - 1u); }

// whether every key of such a result exists; the one refusal of the three finishing entry points
int det_key_fits(const char *who, int n_levels, int max_rows, int max_cols, uint32_t out_capacity) {
    if (n_levels <= (1 << DET_KEY_LEVEL_BITS) && max_rows <= (1 << DET_KEY_ROW_BITS) && max_cols <= (1 << DET_KEY_COL_BITS) &&
        out_capacity <= (1u << DET_KEY_POS_BITS))
        return WB_OK;
    wb_set_error("%s: %d levels of up to %d x %d windows, %u records do not fit the %d/%d/%d/%d-bit key", who, n_levels, max_rows,
                 max_cols, out_capacity, DET_KEY_LEVEL_BITS, DET_KEY_ROW_BITS, DET_KEY_COL_BITS, DET_KEY_POS_BITS);
    return WB_ERR_UNSUPPORTED;
}

// ---- the shard counters, as every lane of a wave sees them (lane = shard)
struct ShardPrefix {
    uint32_t mine;      // valid records of shard `lane`: its counter, clamped to cap
    uint32_t before;    // valid records of the shards in front of it = packed position of its first record
    uint32_t total;     // valid records of all shards
    uint32_t worst;     // fullest raw counter (> cap: records were dropped)
};
__device__ inline ShardPrefix shard_prefix(const uint32_t *det_count, uint32_t cap, int lane) {
    const uint32_t raw = det_count[lane];
    ShardPrefix p = {raw < cap ? raw : cap, 0u, 0u, 0u};
#pragma unroll
    for (int s = 0; s < WB_DET_SHARDS; ++s) {
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)p.mine, s);
        const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)raw, s);
        p.before += s < lane ? c : 0u;
        p.total += c;
        p.worst = r > p.worst ? r : p.worst;
    }
    return p;
}
__device__ inline uint32_t of_shard(uint32_t per_lane, int shard) { return (uint32_t)__builtin_amdgcn_readlane((int)per_lane, shard); }

// the 4-word header in front of packed records or of a finish block
__device__ inline void det_header(int32_t *out, const ShardPrefix &p, uint32_t out_cap, uint32_t fourth) {
    out[0] = (int32_t)p.total;                                    // valid records in all shards
    out[1] = (int32_t)p.worst;                                    // fullest shard (> cap: records were dropped, scan again)
    out[2] = (int32_t)(p.total < out_cap ? p.total : out_cap);    // records present behind this header
    out[3] = (int32_t)fourth;
}

// ---- a finish block: header | keys[out_cap] | boxes[out_cap] | scores[out_cap] in ONE buffer, which the host reads back
//      with one copy (readback.FinishBlock)
struct FinishBlock {
    unsigned long long *keys;
    float4 *boxes;
    float *scores;
    __device__ FinishBlock(int32_t *out, uint32_t out_cap)
        : keys(reinterpret_cast<unsigned long long *>(out + 4)), boxes(reinterpret_cast<float4 *>(keys + out_cap)),
          scores(reinterpret_cast<float *>(boxes + out_cap)) {}
};

// The unordered finish, one workgroup of 256 per shard: for every valid record of the shard, at its packed position
// `at` < out_cap, keys[at] = det_key(level, r, c, at), boxes[at] = window_box, scores[at] = score.  The host sorts the keys and
// gathers -- no per-field arithmetic on the host.
__device__ inline void finish_shard(const WbDet *det, uint32_t cap, int shard, const ShardPrefix &p, const float *inv_scale, int m, int n,
                                    const FinishBlock &o, uint32_t out_cap) {
    const uint32_t cnt = of_shard(p.mine, shard), b0 = of_shard(p.before, shard);
    const WbDet *src = det + (size_t)shard * cap;
    for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
        const uint32_t at = b0 + i;
        if (at >= out_cap) break;
        const WbDet d = src[i];
        o.keys[at] = det_key((uint32_t)d.level, d.r, d.c, at);
        o.boxes[at] = window_box(inv_scale[(uint32_t)d.level], d.r, d.c, m, n);
        o.scores[at] = d.score;
    }
}

// ---- packed position -> record: the prefix sums in LDS (sbefore[64] = total) ...
__device__ inline void store_prefix(uint32_t *sbefore, const ShardPrefix &p) {
    if (threadIdx.x < 64) sbefore[threadIdx.x] = p.before;
    if (threadIdx.x == 0) sbefore[64] = p.total;
}
// ... and where packed position q lies: in the last shard s with sbefore[s] <= q (empty shards share a prefix with their
// successor and are stepped over: the LAST such shard is the one that holds records)
__device__ inline const WbDet *locate(const uint32_t *sbefore, const WbDet *det, uint32_t cap, uint32_t q) {
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = 32; step > 0; step >>= 1)
        if (sbefore[lo + step] <= q) lo += step;
    return det + (size_t)lo * cap + (q - sbefore[lo]);
}

__global__ void boxes_kernel(const WbDet *det, int64_t n_det, const float *inv_scale, int m, int n,
                             float *boxes, float *scores) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_det) return;
    WbDet d = det[i];
    reinterpret_cast<float4 *>(boxes)[i] = window_box(inv_scale[(uint32_t)d.level], d.r, d.c, m, n);
    scores[i] = d.score;
}

// The valid records of all detection shards, back to back behind the header -- what a host read-back or a collective
// wants: ONE contiguous prefix whose length the header gives.  One workgroup per shard; every workgroup reads all
// WB_DET_SHARDS counters (256 B) and derives its own output offset, so there is no second pass.
__global__ __launch_bounds__(256) void det_pack_kernel(const WbDet *det, const uint32_t *det_count, uint32_t cap,
                                                        int32_t *out, uint32_t out_cap) {
    const int shard = blockIdx.x;
    const ShardPrefix p = shard_prefix(det_count, cap, threadIdx.x & 63);
    if (shard == 0 && threadIdx.x == 0) det_header(out, p, out_cap, cap);
    const uint32_t n = of_shard(p.mine, shard), before = of_shard(p.before, shard);
    const uint4 *src = reinterpret_cast<const uint4 *>(det + (size_t)shard * cap);
    uint4 *dst = reinterpret_cast<uint4 *>(out) + 1;
    for (uint32_t i = threadIdx.x; i < n; i += 256)
        if (before + i < out_cap) dst[before + i] = src[i];
}

// Model.detect's last step on the device, unordered (finish_shard); header[3] = cap
__global__ __launch_bounds__(256) void det_finish_kernel(const WbDet *det, const uint32_t *det_count, uint32_t cap,
                                                          const float *inv_scale, int m, int n, int32_t *out, uint32_t out_cap) {
    const ShardPrefix p = shard_prefix(det_count, cap, threadIdx.x & 63);
    if (blockIdx.x == 0 && threadIdx.x == 0) det_header(out, p, out_cap, cap);
    finish_shard(det, cap, blockIdx.x, p, inv_scale, m, n, FinishBlock(out, out_cap), out_cap);
}

// det_finish_kernel with the ordering done here as well (wb_det_finish_sorted_launch).  The keys are unique, so a record's
// place in the reference's order is the NUMBER OF SMALLER KEYS: every workgroup gathers all n <= WB_FINISH_SORT_MAX keys
// into LDS (50 KB of L2 reads, every load in flight at once: a thread finds the shard of its flat index by bisection of
// the shards' prefix sums), ranks its own 16 records against them -- sixteen threads per record, each over a sixteenth of
// the keys, the keys as LDS broadcast reads -- and writes key, box and score straight to the record's rank: up to 256
// workgroups of 16 records, one per CU.  (One workgroup sorting in LDS -- a bitonic network, built first --
// took 37 us for the same: 78 stages x 64 KB through ONE CU's LDS.)  The host takes slices instead of sorting and
// gathering (0.03 ms of a 0.23 ms Model.detect call, and the step that bounded Model.detect_stream at batch 1).
// header[3] = 1 says so.  More valid records than WB_FINISH_SORT_MAX (or than out_cap): the sections are written
// unordered, exactly as det_finish_kernel leaves them, header[3] = 0.
#define WB_FINISH_SORT_MAX 4096
// TPR threads per record, 256 / TPR records per workgroup, WB_FINISH_SORT_MAX * TPR / 256 workgroups (>= WB_DET_SHARDS: the
// unordered form wants a workgroup per shard).  One image: TPR = 16, 256 workgroups -- the latency of Model.detect's last
// step; a batch: TPR = 4, 64 workgroups per image (every workgroup gathers all of its image's keys: fewer, longer ones).
// blockIdx.y: the image of a batch (wb_det_order_batch_launch) -- its own 64 counters, record region and output block
// (img_det / img_out: their distances in records / int32 words); a single image launches one row.
template <int TPR>
__global__ __launch_bounds__(256) void det_finish_sorted_kernel(const WbDet *det, const uint32_t *det_count, uint32_t cap,
                                                                 const float *inv_scale, int m, int n, int32_t *out, uint32_t out_cap,
                                                                 size_t img_det, size_t img_out, const int32_t *tail, uint32_t tail_words) {
    static_assert(WB_FINISH_SORT_MAX * TPR / 256 >= WB_DET_SHARDS, "a workgroup per shard for the unordered form");
    __shared__ unsigned long long skey[WB_FINISH_SORT_MAX];
    __shared__ float sscore[WB_FINISH_SORT_MAX];
    __shared__ uint32_t sbefore[65];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wg = blockIdx.x;
    det_count += (size_t)blockIdx.y * WB_DET_SHARDS;
    det += (size_t)blockIdx.y * img_det;
    out += (size_t)blockIdx.y * img_out;
    // the caller's tail words (the scan's alive[] statistics) behind the scores: ONE read-back carries everything
    if (tail != nullptr)
        for (uint32_t i = (uint32_t)wg * 256u + (uint32_t)tid; i < tail_words; i += gridDim.x * 256u) out[4 + 7 * (size_t)out_cap + i] = tail[i];
    const ShardPrefix p = shard_prefix(det_count, cap, lane);
    const uint32_t total = p.total;
    const bool ordered = total <= out_cap && total <= WB_FINISH_SORT_MAX;
    if (wg == 0 && tid == 0) det_header(out, p, out_cap, ordered ? 1u : 0u);
    const FinishBlock o(out, out_cap);
    if (!ordered) {                                           // (grid-uniform)
        if (wg < WB_DET_SHARDS) finish_shard(det, cap, wg, p, inv_scale, m, n, o, out_cap);
        return;
    }
    constexpr int RPW = 256 / TPR;
    if (total <= (uint32_t)(RPW * wg)) return;                // (this workgroup's records start behind the last one)
    store_prefix(sbefore, p);
    __syncthreads();
    // all keys into LDS: WB_FINISH_SORT_MAX / 256 records per thread, every load requested before the first is used
    constexpr int PER = WB_FINISH_SORT_MAX / 256;
    {
        uint4 lr[PER];                                        // (image, level, r | c << 16, score)
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            // (unconditional: positions past the end load the last record again -- with a branch around it every
            // bisection, six dependent LDS reads, ran alone: sixteen of them in a row were a quarter of the kernel)
            const uint32_t q = (uint32_t)tid + 256u * k;
            lr[k] = *reinterpret_cast<const uint4 *>(locate(sbefore, det, cap, q < total ? q : total - 1u));
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t q = (uint32_t)tid + 256u * k;
            if (q < total) {
                skey[q] = det_key(lr[k].y, lr[k].z & 0xffffu, lr[k].z >> 16, q);
                sscore[q] = __uint_as_float(lr[k].w);        // (the record's second visit below needs no memory)
            }
        }
    }
    __syncthreads();
    // TPR threads per record, each over the keys j = part, part + TPR, ... (a wave's records read the same TPR keys at a
    // time: LDS broadcasts), eight keys per thread and pass in flight
    constexpr uint32_t UN = 8;
    const uint32_t q = (uint32_t)(RPW * wg) + (uint32_t)tid / TPR, part = (uint32_t)tid % TPR;
    const bool live = q < total;
    const unsigned long long me = skey[live ? q : 0u];
    uint32_t smaller = 0;
    const uint32_t nfull = total - total % (TPR * UN);        // whole passes; the rest key by key
    for (uint32_t j = part; j < nfull; j += TPR * UN) {
        unsigned long long kk[UN];
#pragma unroll
        for (uint32_t u = 0; u < UN; ++u) kk[u] = skey[j + TPR * u];
#pragma unroll
        for (uint32_t u = 0; u < UN; ++u) smaller += kk[u] < me ? 1u : 0u;
    }
    for (uint32_t j = nfull + part; j < total; j += TPR) smaller += skey[j] < me ? 1u : 0u;
#pragma unroll
    for (uint32_t d = 1; d < TPR; d <<= 1) smaller += (uint32_t)__shfl_xor((int)smaller, (int)d);
    if (live && part == 0) {
        o.keys[smaller] = me;
        o.boxes[smaller] = window_box(inv_scale[det_key_level(me)], det_key_row(me), det_key_col(me), m, n);
        o.scores[smaller] = sscore[q];
    }
}

// A batch's detections by image (the step in front of det_finish_sorted_kernel for a batch): workgroup b walks ALL valid
// records of the shards -- flat positions, the shard of a position by bisection of the prefix sums, several loads in
// flight per thread -- and appends those of image b to bucket b (wave-aggregated: one LDS atomic per wave and pass).
// The order inside a bucket is whatever the atomics gave; ranking by key does not depend on it.  bucket_count[b][0] =
// the image's record count (above bucket_cap: the finishing kernel reports the overflow), [b][1..63] = 0: a bucket reads
// as a shard set whose first shard holds everything.  info = (valid records, fullest shard, images, bucket_cap).
__global__ __launch_bounds__(1024) void det_bucket_kernel(const WbDet *det, const uint32_t *det_count, uint32_t cap, WbDet *bucket,
                                                           uint32_t bucket_cap, uint32_t *bucket_count, int32_t *info) {
    __shared__ uint32_t sbefore[65];
    __shared__ uint32_t n_img;
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    const ShardPrefix p = shard_prefix(det_count, cap, lane);
    const uint32_t total = p.total;
    if (b == 0 && tid == 0) {
        info[0] = (int32_t)total;
        info[1] = (int32_t)p.worst;
        info[2] = (int32_t)gridDim.x;
        info[3] = (int32_t)bucket_cap;
    }
    store_prefix(sbefore, p);
    if (tid == 0) n_img = 0;
    __syncthreads();
    WbDet *dst = bucket + (size_t)b * bucket_cap;
    constexpr int U = 4;
    for (uint32_t q0 = 0; q0 < total; q0 += 1024 * U) {      // (workgroup-uniform bounds)
        uint4 rec[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t q = q0 + (uint32_t)tid + 1024u * u;
            ok[u] = q < total;
            rec[u] = make_uint4(0xffffffffu, 0u, 0u, 0u);
            if (ok[u]) rec[u] = *reinterpret_cast<const uint4 *>(locate(sbefore, det, cap, q));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool take = ok[u] && (int)rec[u].x == b;
            const unsigned long long mask = __ballot(take);
            if (mask == 0ull) continue;                       // (wave-uniform)
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&n_img, (uint32_t)__popcll(mask));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (take) {
                // the takers in front of this lane (mbcnt: never a 64-bit shift by a lane's own amount)
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                const uint32_t slot = base + rank;
                if (slot < bucket_cap) *reinterpret_cast<uint4 *>(dst + slot) = rec[u];
            }
        }
    }
    __syncthreads();
    if (tid < 64) bucket_count[(size_t)b * WB_DET_SHARDS + tid] = tid == 0 ? n_img : 0u;
}

}  // namespace

extern "C" int wb_boxes_launch(void *stream, const WbDet *det, int64_t n_det, const float *inv_scale, int m,
                               int n, float *boxes, float *scores) {
    WB_REQUIRE(n_det >= 0, "wb_boxes_launch: negative count");
    if (n_det == 0) return WB_OK;
    WB_REQUIRE(det && inv_scale && boxes && scores, "wb_boxes_launch: null pointer");
    int64_t blocks = (n_det + 255) / 256;
    hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, det, n_det,
                       inv_scale, m, n, boxes, scores);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_det_pack_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                                  int32_t *packed, uint32_t packed_capacity) {
    WB_REQUIRE(det_count && packed, "wb_det_pack_launch: null pointer");
    WB_REQUIRE(det || shard_capacity == 0, "wb_det_pack_launch: det is null but capacity > 0");
    WB_REQUIRE(wb_aligned(packed, 16), "wb_det_pack_launch: packed must be 16-byte aligned");
    hipLaunchKernelGGL(det_pack_kernel, dim3(WB_DET_SHARDS), dim3(256), 0, (hipStream_t)stream, det, det_count,
                       shard_capacity, packed, packed_capacity);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_det_finish_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                                    const float *inv_scale, int n_levels, int max_rows, int max_cols, int m, int n,
                                    void *out, uint32_t out_capacity) {
    WB_REQUIRE(det_count && out && inv_scale, "wb_det_finish_launch: null pointer");
    WB_REQUIRE(det || shard_capacity == 0, "wb_det_finish_launch: det is null but capacity > 0");
    WB_REQUIRE(wb_aligned(out, 16), "wb_det_finish_launch: out must be 16-byte aligned");
    WB_REQUIRE(out_capacity % 2 == 0, "wb_det_finish_launch: out_capacity must be even (16-byte aligned sections)");
    if (int rc = det_key_fits("wb_det_finish_launch", n_levels, max_rows, max_cols, out_capacity)) return rc;
    hipLaunchKernelGGL(det_finish_kernel, dim3(WB_DET_SHARDS), dim3(256), 0, (hipStream_t)stream, det, det_count,
                       shard_capacity, inv_scale, m, n, reinterpret_cast<int32_t *>(out), out_capacity);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_det_finish_sorted_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                                           const float *inv_scale, int n_levels, int max_rows, int max_cols, int m, int n,
                                           void *out, uint32_t out_capacity, const int32_t *tail, uint32_t tail_words) {
    WB_REQUIRE(tail || tail_words == 0, "wb_det_finish_sorted_launch: tail is null but tail_words > 0");
    WB_REQUIRE(det_count && out && inv_scale, "wb_det_finish_sorted_launch: null pointer");
    WB_REQUIRE(det || shard_capacity == 0, "wb_det_finish_sorted_launch: det is null but capacity > 0");
    WB_REQUIRE(wb_aligned(out, 16), "wb_det_finish_sorted_launch: out must be 16-byte aligned");
    WB_REQUIRE(out_capacity % 2 == 0, "wb_det_finish_sorted_launch: out_capacity must be even (16-byte aligned sections)");
    if (int rc = det_key_fits("wb_det_finish_sorted_launch", n_levels, max_rows, max_cols, out_capacity)) return rc;
    hipLaunchKernelGGL(det_finish_sorted_kernel<16>, dim3(WB_FINISH_SORT_MAX * 16 / 256), dim3(256), 0, (hipStream_t)stream, det, det_count,
                       shard_capacity, inv_scale, m, n, reinterpret_cast<int32_t *>(out), out_capacity, (size_t)0, (size_t)0, tail, tail_words);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}

extern "C" int wb_det_order_batch_launch(void *stream, const WbDet *det, const uint32_t *det_count, uint32_t shard_capacity,
                                         int n_images, const float *inv_scale, int n_levels, int max_rows, int max_cols, int m,
                                         int n, void *scratch, size_t scratch_bytes, void *out, uint32_t out_capacity) {
    WB_REQUIRE(det_count && out && inv_scale && scratch, "wb_det_order_batch_launch: null pointer");
    WB_REQUIRE(det || shard_capacity == 0, "wb_det_order_batch_launch: det is null but capacity > 0");
    WB_REQUIRE(n_images >= 1 && n_images <= 65535, "wb_det_order_batch_launch: 1 .. 65535 images");
    WB_REQUIRE(wb_aligned(out, 16) && wb_aligned(scratch, 16),
               "wb_det_order_batch_launch: out and scratch must be 16-byte aligned");
    WB_REQUIRE(out_capacity % 4 == 0 && out_capacity >= 4, "wb_det_order_batch_launch: out_capacity must be a multiple of 4 (16-byte aligned blocks)");
    if (int rc = det_key_fits("wb_det_order_batch_launch", n_levels, max_rows, max_cols, out_capacity)) return rc;
    const size_t counts_bytes = (size_t)n_images * WB_DET_SHARDS * 4, need = counts_bytes + (size_t)n_images * out_capacity * sizeof(WbDet);
    if (scratch_bytes < need) {
        wb_set_error("wb_det_order_batch_launch: scratch holds %zu bytes, %d images of %u records want %zu", scratch_bytes, n_images,
                     out_capacity, need);
        return WB_ERR_INVALID;
    }
    uint32_t *bucket_count = reinterpret_cast<uint32_t *>(scratch);
    WbDet *bucket = reinterpret_cast<WbDet *>(reinterpret_cast<unsigned char *>(scratch) + counts_bytes);
    int32_t *info = reinterpret_cast<int32_t *>(out);
    hipLaunchKernelGGL(det_bucket_kernel, dim3(n_images), dim3(1024), 0, (hipStream_t)stream, det, det_count, shard_capacity, bucket,
                       out_capacity, bucket_count, info);
    hipLaunchKernelGGL(det_finish_sorted_kernel<4>, dim3(WB_FINISH_SORT_MAX * 4 / 256, n_images), dim3(256), 0, (hipStream_t)stream, bucket, bucket_count,
                       out_capacity, inv_scale, m, n, info + 4, out_capacity, (size_t)out_capacity, (size_t)(4 + 7 * (size_t)out_capacity),
                       (const int32_t *)nullptr, 0u);
    WB_HIP_CHECK(hipGetLastError());
    return WB_OK;
}
