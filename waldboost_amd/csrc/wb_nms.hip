// Greedy non-maximum suppression on the device (wb_nms_launch, wb_nms_finish_launch): the step every caller of
// Model.detect runs next (reference testing.py:46 bbx.non_max_suppression, scripts/waldboost-detect.py:36).
//
// Semantics (tests/nms_reference.py is the NumPy statement):
//   * boxes with `not (score >= score_threshold)` are dropped first (when a score threshold is given);
//   * visiting order: score descending, -0.0 == +0.0, equal scores in INPUT ORDER (np.argsort(-scores, kind="stable"));
//   * a box is kept unless an already kept box of its group has iou > iou_threshold with it (strict);
//   * iou is boxes.iou's float64 arithmetic on the float32 coordinates, operation by operation (this file is built with
//     -ffp-contract=off: no fused multiply-add; the float64 divide is the correctly rounded one);
//   * the result is a keep flag per box, in input order.
//
// Four kernels, all addressed by "sorted position" p (the place of a box in the visiting order):
//   nms_rank_kernel     p(i) = number of boxes whose (key(score), input order, index) is smaller -- the triples are
//                       unique, so counting IS the stable sort.  Writes order[p] = i and the box, group and dropped flag
//                       at p.  Quadratic: wb_nms_launch takes it up to 2^16 boxes.
//   nms_gather_kernel   the same writes from a visiting order the caller computed (wb_nms_ordered_launch: any n).
//   nms_matrix_kernel   one wave per 64 x 64 block of (row p_i, column p_j > p_i) pairs of a BAND of rows: box i from
//                       LDS, one column per lane, __ballot gives row i's 64-bit word.  Upper triangle only.
//   nms_scan_kernel     ONE wave walks the band's rows in order.  Lane l holds word l of the band's "removed" window
//                       (bands are at most 4096 rows = 64 words).  Per 64 rows: the diagonal block is resolved in
//                       registers (row r's word from lane r, scalar arithmetic), then the kept rows' words are ORed
//                       into the lanes behind.  Only kept rows cost a row read.
//   nms_spread_kernel   (more than one band) ORs the band's kept rows into the removed bitmap of the columns behind the
//                       band, which the later bands start from.
// A band is as many rows (a multiple of 64, at most 4096) as the caller's scratch holds matrix rows for.
#include "wb_common.h"

#define WB_NMS_BAND 4096            // most rows of a band: the scan wave's window, one 64-bit word per lane
#define WB_NMS_MAX (1 << 16)        // most boxes of one wb_nms_launch (the rank pass is quadratic)
#define WB_NMS_ORDERED_MAX (1 << 26) // most boxes of one wb_nms_ordered_launch (what a finish buffer's key can count)
#define WB_NMS_FINISH_MAX 4096      // most boxes of one image of wb_nms_finish_launch (one band, sized before n is known)
#define WB_NMS_MATRIX_BUDGET ((size_t)64 << 20)

namespace {

struct NmsLayout {                  // byte offsets inside one problem's scratch, for at most n_max boxes
    uint32_t n64, W;                // n_max rounded up to 64; words per matrix row
    size_t sbox, sgroup, order, sdead, removed, kept, cnt, matrix, fixed_end;
};

NmsLayout nms_layout(size_t n_max) {
    NmsLayout L;
    L.n64 = (uint32_t)((n_max + 63) / 64 * 64);
    if (L.n64 == 0) L.n64 = 64;
    L.W = L.n64 / 64;
    size_t o = 0;
    L.sbox = o;    o += (size_t)L.n64 * 16;
    L.sgroup = o;  o += (size_t)L.n64 * 4;
    L.order = o;   o += (size_t)L.n64 * 4;
    L.sdead = o;   o += (size_t)L.n64;
    L.removed = o; o += (size_t)L.W * 8;
    L.kept = o;    o += (size_t)L.W * 8;
    L.cnt = o;     o += 16;
    o = (o + 255) / 256 * 256;
    L.matrix = o;
    L.fixed_end = o;
    return L;
}

struct NmsArgs {
    // finish form: image b's block header | keys | boxes | scores at fin + b * fin_stride (bytes), capacity cap
    const uint8_t *fin;
    size_t fin_stride;
    uint32_t cap;
    // plain form (fin == nullptr)
    const float4 *boxes;
    const float *scores;
    const int32_t *group;
    const uint32_t *visit;          // wb_nms_ordered_launch: the caller's visiting order (nullptr: nms_rank_kernel finds it)
    uint32_t n;
    double thr;
    int use_st;
    float st;
    uint8_t *scratch;               // problem b's at scratch + b * scratch_stride
    size_t scratch_stride;
    NmsLayout L;
    uint32_t R;                     // rows per band
    uint8_t *keep;                  // plain: uint8 [n]; finish: image b's uint32 info[4] | uint8 keep[cap] at keep + b * (16 + cap)
    uint32_t *n_keep;               // plain
};

struct NmsView {
    uint32_t n;
    bool done;                      // finish form: the image's detections are all present and at most WB_NMS_FINISH_MAX
    bool by_key;                    // finish form, sections in packed order: the input order is the key order
    const float4 *boxes;
    const float *scores;
    const int32_t *group;
    const unsigned long long *keys;
    float4 *sbox;
    int32_t *sgroup;
    uint32_t *order;
    uint8_t *sdead;
    unsigned long long *removed, *kept, *matrix;
    uint32_t *cnt;
    uint8_t *keep;
    uint32_t *info;                 // finish form: info[4] in front of the keep flags
};

__device__ inline NmsView nms_view(const NmsArgs &a, uint32_t b) {
    NmsView v;
    uint8_t *s = a.scratch + (size_t)b * a.scratch_stride;
    v.sbox = reinterpret_cast<float4 *>(s + a.L.sbox);
    v.sgroup = reinterpret_cast<int32_t *>(s + a.L.sgroup);
    v.order = reinterpret_cast<uint32_t *>(s + a.L.order);
    v.sdead = s + a.L.sdead;
    v.removed = reinterpret_cast<unsigned long long *>(s + a.L.removed);
    v.kept = reinterpret_cast<unsigned long long *>(s + a.L.kept);
    v.cnt = reinterpret_cast<uint32_t *>(s + a.L.cnt);
    v.matrix = reinterpret_cast<unsigned long long *>(s + a.L.matrix);
    if (a.fin == nullptr) {
        v.n = a.n;
        v.done = true;
        v.by_key = false;
        v.boxes = a.boxes;
        v.scores = a.scores;
        v.group = a.group;
        v.keys = nullptr;
        v.keep = a.keep;
        v.info = nullptr;
        return v;
    }
    const uint8_t *blk = a.fin + (size_t)b * a.fin_stride;
    const int32_t *hdr = reinterpret_cast<const int32_t *>(blk);
    const uint32_t total = (uint32_t)hdr[0];
    v.done = total <= a.cap && total <= WB_NMS_FINISH_MAX;
    v.n = v.done ? total : 0u;
    v.by_key = hdr[3] == 0;
    v.keys = reinterpret_cast<const unsigned long long *>(blk + 16);
    v.boxes = reinterpret_cast<const float4 *>(blk + 16 + 8 * (size_t)a.cap);
    v.scores = reinterpret_cast<const float *>(blk + 16 + 24 * (size_t)a.cap);
    v.group = nullptr;
    v.info = reinterpret_cast<uint32_t *>(a.keep + (size_t)b * (16 + (size_t)a.cap));
    v.keep = reinterpret_cast<uint8_t *>(v.info + 4);
    return v;
}

// descending score as an ascending 32-bit word; the two zeros are one value
__device__ inline uint32_t nms_score_word(float s) {
    if (s == 0.0f) s = 0.0f;
    return ~wb_f32_key(s);
}

__device__ inline unsigned long long nms_readlane64(unsigned long long x, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ inline unsigned long long nms_uniform64(unsigned long long x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// ---- order: rank by counting ----
__global__ __launch_bounds__(256) void nms_rank_kernel(NmsArgs a) {
    __shared__ uint32_t shi[256];
    __shared__ unsigned long long slo[256];
    const NmsView v = nms_view(a, blockIdx.y);
    const uint32_t n = v.n, tid = threadIdx.x;
    if (blockIdx.x * 256u >= n) return;                        // (workgroup-uniform)
    const uint32_t i = blockIdx.x * 256u + tid;
    const bool live = i < n;
    const uint32_t ii = live ? i : n - 1u;
    const float sc = v.scores[ii];
    const uint32_t hi = nms_score_word(sc);
    const unsigned long long lo = v.by_key ? v.keys[ii] : (unsigned long long)ii;
    uint32_t smaller = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 256u) {
        const uint32_t j = t0 + tid;
        __syncthreads();
        if (j < n) {
            shi[tid] = nms_score_word(v.scores[j]);
            slo[tid] = v.by_key ? v.keys[j] : (unsigned long long)j;
        }
        __syncthreads();
        const uint32_t m = n - t0 < 256u ? n - t0 : 256u;
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t hj = shi[k];
            const unsigned long long lj = slo[k];
            // (the index last: the ranks are a permutation whatever the keys hold)
            smaller += (hj < hi || (hj == hi && (lj < lo || (lj == lo && t0 + k < i)))) ? 1u : 0u;
        }
    }
    if (live) {                                                // smaller < n: the triples are unique
        v.order[smaller] = i;
        v.sbox[smaller] = v.boxes[i];
        v.sgroup[smaller] = v.group ? v.group[i] : 0;
        v.sdead[smaller] = (a.use_st && !(sc >= a.st)) ? 1 : 0;
    }
}

// ---- order given by the caller: position p visits box visit[p] ----
__global__ __launch_bounds__(256) void nms_gather_kernel(NmsArgs a) {
    const NmsView v = nms_view(a, 0);
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= v.n) return;
    const uint32_t i = a.visit[p];
    const bool ok = i < v.n;                                   // (an index outside the arrays: never read, never kept)
    const uint32_t ii = ok ? i : 0u;
    v.order[p] = ok ? i : 0xffffffffu;
    v.sbox[p] = v.boxes[ii];
    v.sgroup[p] = v.group ? v.group[ii] : 0;
    v.sdead[p] = (!ok || (a.use_st && !(v.scores[ii] >= a.st))) ? 1 : 0;
}

// ---- suppression matrix of the band of rows [r0, r0 + R): word (p_i - r0) * W + p_j / 64, bit p_j % 64 ----
__global__ __launch_bounds__(256) void nms_matrix_kernel(NmsArgs a, uint32_t r0) {
    __shared__ float4 sb[64];
    __shared__ int32_t sg[64];
    const NmsView v = nms_view(a, blockIdx.z);
    const uint32_t n = v.n, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t rc = r0 / 64u + blockIdx.y;                 // chunk of 64 rows
    if (rc * 64u >= n) return;                                 // (workgroup-uniform)
    if (tid < 64u) {
        const uint32_t p = rc * 64u + tid < n ? rc * 64u + tid : n - 1u;
        sb[tid] = v.sbox[p];
        sg[tid] = v.sgroup[p];
    }
    __syncthreads();
    const uint32_t jc = blockIdx.x * 4u + wave, Wn = (n + 63u) / 64u;
    if (jc < rc || jc >= Wn) return;                           // (wave-uniform) lower triangle, or behind the last box
    const uint32_t j = jc * 64u + lane, jj = j < n ? j : n - 1u;
    const float4 bj = v.sbox[jj];
    const int32_t gj = v.sgroup[jj];
    const double bx1 = (double)bj.x, by1 = (double)bj.y, bx2 = (double)bj.z, by2 = (double)bj.w;
    const double area_b = (bx2 - bx1) * (by2 - by1);
    const double thr = a.thr;
    unsigned long long word = 0ull;
    for (uint32_t r = 0; r < 64u; ++r) {
        const float4 bi = sb[r];
        const double ax1 = (double)bi.x, ay1 = (double)bi.y, ax2 = (double)bi.z, ay2 = (double)bi.w;
        // boxes.iou, operation by operation
        double iw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1);
        double ih = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1);
        iw = iw < 0.0 ? 0.0 : iw;
        ih = ih < 0.0 ? 0.0 : ih;
        const double inter = iw * ih;
        const double area_a = (ax2 - ax1) * (ay2 - ay1);
        const double uni = area_a + area_b - inter;
        const double iou = uni > 0.0 ? inter / uni : 0.0;
        const uint32_t i = rc * 64u + r;
        const bool hit = iou > thr && sg[r] == gj && j > i && j < n;
        const unsigned long long m = __ballot(hit);
        if (lane == r) word = m;
    }
    // (rows behind the last box hold zeros: j > i >= n never holds with j < n)
    v.matrix[(size_t)(rc * 64u - r0 + lane) * a.L.W + jc] = word;
}

// ---- the greedy scan of one band ----
__global__ __launch_bounds__(64) void nms_scan_kernel(NmsArgs a, uint32_t r0, int first, int last) {
    const NmsView v = nms_view(a, blockIdx.y);
    const uint32_t n = v.n, lane = threadIdx.x;
    const uint32_t n64 = (n + 63u) / 64u * 64u, Wn = n64 / 64u, W = a.L.W;
    const uint32_t w0 = r0 / 64u;
    uint32_t Rw = 0;                                           // chunks of 64 rows in this band
    if (r0 < n64) Rw = (n64 - r0 < a.R ? n64 - r0 : a.R) / 64u;
    // the window: dropped boxes and the padding behind the last box are removed from the start; later bands add what the
    // earlier bands' kept rows removed
    unsigned long long win = ~0ull;
    for (uint32_t c = 0; c < Rw; ++c) {
        const uint32_t p = r0 + 64u * c + lane;
        const bool dead = p >= n || v.sdead[p] != 0;
        unsigned long long m = __ballot(dead);
        if (!first) m |= nms_uniform64(v.removed[w0 + c]);
        if (lane == c) win = m;
    }
    if (first)
        for (uint32_t w = w0 + Rw + lane; w < Wn; w += 64u) v.removed[w] = 0ull;
    uint32_t total = first ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)v.cnt[0]);
    unsigned long long keptw = 0ull;
    for (uint32_t c = 0; c < Rw; ++c) {
        // the diagonal block: row r's word in lane r; resolved with scalar arithmetic
        const unsigned long long D = v.matrix[(size_t)(64u * c + lane) * W + w0 + c];
        unsigned long long rem = nms_readlane64(win, (int)c), kept = 0ull;
#pragma unroll
        for (int r = 0; r < 64; ++r) {
            const unsigned long long bit = 1ull << r;          // (a constant)
            const unsigned long long row = nms_readlane64(D, r);
            if (!(rem & bit)) {
                kept |= bit;
                rem |= row;
            }
        }
        if (lane == c) keptw = kept;
        total += (uint32_t)__popcll(kept);
        // the kept rows' words into the window words behind this chunk, four loads in flight
        const bool behind = lane > c && lane < Rw;
        unsigned long long m = kept;
        while (m != 0ull) {                                    // (wave-uniform)
            unsigned long long x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                x[u] = 0ull;
                if (m != 0ull) {
                    const uint32_t r = (uint32_t)__ffsll((long long)m) - 1u;
                    m &= m - 1ull;
                    if (behind) x[u] = v.matrix[(size_t)(64u * c + r) * W + w0 + lane];
                }
            }
            win |= (x[0] | x[1]) | (x[2] | x[3]);
        }
    }
    if (lane < Rw) v.kept[w0 + lane] = keptw;
    // keep flags in input order (a lane's bit from the 32-bit half it lies in)
    for (uint32_t c = 0; c < Rw; ++c) {
        const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)keptw, (int)c);
        const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(keptw >> 32), (int)c);
        const uint32_t half = lane >= 32u ? khi : klo;     // (never a 64-bit shift by a lane's own amount)
        const uint32_t p = r0 + 64u * c + lane;
        if (p < n) {
            const uint32_t i = v.order[p];
            if (i < n) v.keep[i] = (uint8_t)((half >> (lane & 31u)) & 1u);
        }
    }
    if (lane == 0) {
        v.cnt[0] = total;
        if (last) {
            if (v.info) {
                v.info[0] = total;
                v.info[1] = n;
                v.info[2] = v.done ? 1u : 0u;
                v.info[3] = 0u;
            } else {
                a.n_keep[0] = total;
            }
        }
    }
}

// ---- what a band's kept rows remove behind the band ----
__global__ __launch_bounds__(256) void nms_spread_kernel(NmsArgs a, uint32_t r0) {
    const NmsView v = nms_view(a, blockIdx.z);
    const uint32_t n = v.n, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n64 = (n + 63u) / 64u * 64u, Wn = n64 / 64u, W = a.L.W, w0 = r0 / 64u;
    if (r0 >= n64) return;
    const uint32_t Rw = (n64 - r0 < a.R ? n64 - r0 : a.R) / 64u;
    const uint32_t w = w0 + Rw + blockIdx.x * 64u + lane;
    const bool ok = w < Wn;
    unsigned long long acc = 0ull;
    for (uint32_t c = blockIdx.y * 4u + wave; c < Rw; c += gridDim.y * 4u) {
        unsigned long long m = nms_uniform64(v.kept[w0 + c]);
        while (m != 0ull) {
            const uint32_t r = (uint32_t)__ffsll((long long)m) - 1u;
            m &= m - 1ull;
            if (ok) acc |= v.matrix[(size_t)(64u * c + r) * W + w];
        }
    }
    if (ok && acc != 0ull) atomicOr(&v.removed[w], acc);
}

int nms_enqueue(hipStream_t st, NmsArgs &a, uint32_t n_max, int n_problems) {
    const uint32_t n64 = (n_max + 63u) / 64u * 64u;
    if (n_max > 0) {
        if (a.visit != nullptr)
            hipLaunchKernelGGL(nms_gather_kernel, dim3((n_max + 255u) / 256u), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(nms_rank_kernel, dim3((n_max + 255u) / 256u, n_problems), dim3(256), 0, st, a);
        WB_HIP_CHECK(hipGetLastError());
    }
    const uint32_t Wn = n64 / 64u;
    uint32_t r0 = 0;
    do {
        const uint32_t rows = n64 - r0 < a.R ? n64 - r0 : a.R;
        const int last = r0 + rows >= n64;
        if (rows > 0) {
            hipLaunchKernelGGL(nms_matrix_kernel, dim3((Wn + 3u) / 4u, rows / 64u, n_problems), dim3(256), 0, st, a, r0);
            WB_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(nms_scan_kernel, dim3(1, n_problems), dim3(64), 0, st, a, r0, r0 == 0 ? 1 : 0, last);
        WB_HIP_CHECK(hipGetLastError());
        if (!last) {
            const uint32_t behind = Wn - (r0 + rows) / 64u;
            const uint32_t chunks = rows / 64u;
            hipLaunchKernelGGL(nms_spread_kernel, dim3((behind + 63u) / 64u, (chunks + 3u) / 4u, n_problems), dim3(256), 0, st, a, r0);
            WB_HIP_CHECK(hipGetLastError());
        }
        r0 += rows;
    } while (r0 < n64);
    return WB_OK;
}

size_t nms_matrix_bytes(const NmsLayout &L) {
    const size_t row = (size_t)L.W * 8;
    const size_t rows = L.n64 < WB_NMS_BAND ? L.n64 : WB_NMS_BAND;
    size_t want = rows * row;
    const size_t floor64 = 64 * row;
    const size_t cap = WB_NMS_MATRIX_BUDGET > floor64 ? WB_NMS_MATRIX_BUDGET : floor64;
    return want < cap ? want : cap;
}

}  // namespace

extern "C" int wb_nms_scratch_bytes(int64_t n, size_t *bytes) {
    WB_REQUIRE(bytes != nullptr, "wb_nms_scratch_bytes: null pointer");
    WB_REQUIRE(n >= 0, "wb_nms_scratch_bytes: n = %lld is negative", (long long)n);
    if (n > WB_NMS_ORDERED_MAX) {
        wb_set_error("wb_nms_scratch_bytes: %lld boxes (at most %d in one call)", (long long)n, WB_NMS_ORDERED_MAX);
        return WB_ERR_UNSUPPORTED;
    }
    const NmsLayout L = nms_layout((size_t)n);
    *bytes = L.fixed_end + nms_matrix_bytes(L);
    return WB_OK;
}

extern "C" int wb_nms_finish_scratch_bytes(uint32_t out_capacity, int n_images, size_t *bytes) {
    WB_REQUIRE(bytes != nullptr, "wb_nms_finish_scratch_bytes: null pointer");
    WB_REQUIRE(n_images >= 1 && n_images <= 65535, "wb_nms_finish_scratch_bytes: 1 .. 65535 images");
    const NmsLayout L = nms_layout(out_capacity < WB_NMS_FINISH_MAX ? out_capacity : WB_NMS_FINISH_MAX);
    *bytes = (size_t)n_images * (L.fixed_end + (size_t)L.n64 * L.W * 8);
    return WB_OK;
}

static int nms_check_common(const char *who, double iou_threshold, const void *scratch) {
    WB_REQUIRE(iou_threshold == iou_threshold && iou_threshold >= 0.0, "%s: iou_threshold must be a number >= 0", who);
    WB_REQUIRE(scratch != nullptr, "%s: null pointer", who);
    WB_REQUIRE(wb_aligned(scratch, 16), "%s: scratch must be 16-byte aligned", who);
    return WB_OK;
}

static int nms_plain(const char *who, void *stream, const float *boxes, const float *scores, const int32_t *group,
                     const uint32_t *visit, bool ordered, int64_t n, int64_t n_most, double iou_threshold, int use_score_threshold,
                     float score_threshold, void *scratch, size_t scratch_bytes, uint8_t *keep, uint32_t *n_keep) {
    WB_REQUIRE(n >= 0, "%s: n = %lld is negative", who, (long long)n);
    if (int rc = nms_check_common(who, iou_threshold, scratch)) return rc;
    WB_REQUIRE(n_keep != nullptr && (n == 0 || (boxes && scores && keep && (visit || !ordered))), "%s: null pointer", who);
    WB_REQUIRE(wb_aligned(boxes, 16), "%s: boxes must be 16-byte aligned", who);
    WB_REQUIRE(wb_aligned(scores, 4) && wb_aligned(group, 4) &&
                   wb_aligned(n_keep, 4) && wb_aligned(visit, 4),
               "%s: scores, group, order and n_keep must be 4-byte aligned", who);
    WB_REQUIRE(!use_score_threshold || score_threshold == score_threshold, "%s: score_threshold is NaN", who);
    if (n > n_most) {
        wb_set_error("%s: %lld boxes (at most %lld in one call)", who, (long long)n, (long long)n_most);
        return WB_ERR_UNSUPPORTED;
    }
    NmsArgs a = {};
    a.visit = n > 0 ? visit : nullptr;
    a.L = nms_layout((size_t)n);
    const size_t row = (size_t)a.L.W * 8;
    WB_REQUIRE(scratch_bytes >= a.L.fixed_end + 64 * row,
               "%s: scratch holds %zu bytes, %lld boxes want at least %zu (wb_nms_scratch_bytes)", who, scratch_bytes,
               (long long)n, a.L.fixed_end + 64 * row);
    size_t rows = (scratch_bytes - a.L.fixed_end) / row / 64 * 64;
    if (rows > WB_NMS_BAND) rows = WB_NMS_BAND;
    if (rows > a.L.n64) rows = a.L.n64;
    a.R = (uint32_t)rows;
    a.boxes = reinterpret_cast<const float4 *>(boxes);
    a.scores = scores;
    a.group = group;
    a.n = (uint32_t)n;
    a.thr = iou_threshold;
    a.use_st = use_score_threshold ? 1 : 0;
    a.st = score_threshold;
    a.scratch = static_cast<uint8_t *>(scratch);
    a.keep = keep;
    a.n_keep = n_keep;
    return nms_enqueue((hipStream_t)stream, a, (uint32_t)n, 1);
}

extern "C" int wb_nms_launch(void *stream, const float *boxes, const float *scores, const int32_t *group, int64_t n,
                             double iou_threshold, int use_score_threshold, float score_threshold, void *scratch,
                             size_t scratch_bytes, uint8_t *keep, uint32_t *n_keep) {
    return nms_plain("wb_nms_launch", stream, boxes, scores, group, nullptr, false, n, WB_NMS_MAX, iou_threshold, use_score_threshold,
                     score_threshold, scratch, scratch_bytes, keep, n_keep);
}

extern "C" int wb_nms_ordered_launch(void *stream, const float *boxes, const float *scores, const int32_t *group,
                                     const uint32_t *order, int64_t n, double iou_threshold, int use_score_threshold,
                                     float score_threshold, void *scratch, size_t scratch_bytes, uint8_t *keep, uint32_t *n_keep) {
    return nms_plain("wb_nms_ordered_launch", stream, boxes, scores, group, order, true, n, WB_NMS_ORDERED_MAX, iou_threshold,
                     use_score_threshold, score_threshold, scratch, scratch_bytes, keep, n_keep);
}

extern "C" int wb_nms_finish_launch(void *stream, const void *fin, uint32_t out_capacity, int n_images, double iou_threshold,
                                    int use_score_threshold, float score_threshold, void *scratch, size_t scratch_bytes,
                                    void *result) {
    if (int rc = nms_check_common("wb_nms_finish_launch", iou_threshold, scratch)) return rc;
    WB_REQUIRE(fin != nullptr && result != nullptr, "wb_nms_finish_launch: null pointer");
    WB_REQUIRE(wb_aligned(fin, 16) && wb_aligned(result, 4),
               "wb_nms_finish_launch: fin must be 16-byte, result 4-byte aligned");
    WB_REQUIRE(n_images >= 1 && n_images <= 65535, "wb_nms_finish_launch: 1 .. 65535 images");
    WB_REQUIRE(out_capacity >= 4 && out_capacity % 4 == 0 && out_capacity <= (1u << 26),
               "wb_nms_finish_launch: out_capacity must be a multiple of 4, at most 2^26");
    WB_REQUIRE(!use_score_threshold || score_threshold == score_threshold, "wb_nms_finish_launch: score_threshold is NaN");
    size_t need = 0;
    wb_nms_finish_scratch_bytes(out_capacity, n_images, &need);
    WB_REQUIRE(scratch_bytes >= need, "wb_nms_finish_launch: scratch holds %zu bytes, %d images of up to %u boxes want %zu",
               scratch_bytes, n_images, out_capacity, need);
    const uint32_t n_max = out_capacity < WB_NMS_FINISH_MAX ? out_capacity : WB_NMS_FINISH_MAX;
    NmsArgs a = {};
    a.L = nms_layout(n_max);
    a.R = a.L.n64;
    a.fin = static_cast<const uint8_t *>(fin);
    a.fin_stride = 16 + 28 * (size_t)out_capacity;
    a.cap = out_capacity;
    a.thr = iou_threshold;
    a.use_st = use_score_threshold ? 1 : 0;
    a.st = score_threshold;
    a.scratch = static_cast<uint8_t *>(scratch);
    a.scratch_stride = need / (size_t)n_images;
    a.keep = static_cast<uint8_t *>(result);
    return nms_enqueue((hipStream_t)stream, a, n_max, n_images);
}
