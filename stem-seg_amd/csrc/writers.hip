// Device half of the YouTube-VIS / KITTI-MOTS writers (output_utils/youtube_vis.py:113-161, kitti_mots.py:89-173).
//
// (1) COCO RLE of every (frame, kept instance) binary plane of a condensed index map M[F][H][W] (uint8 / uint16, value n = kept
//     instance n, 0 = none), in pycocotools' conventions (maskApi.c rleEncode / rleToString / rleArea / rleToBbox):
//     column-major order p = x * H + y, counts alternate starting with a (possibly empty) run of zeros and sum to H * W.
//       colcount : one thread per (frame, column) walks its column -- the rows are read row-major, so a wave's 64 loads of one
//                  row are contiguous -- and counts the change points s[p] != s[p-1] (s[-1] = 0); every change point is a
//                  boundary of at most two planes (old value, new value), one "contribution" each
//       scan     : contributions per column -> offsets (three-phase exclusive scan, one tile per workgroup)
//       emit     : the same walk writes (key = f * K + n - 1, p) per contribution: sorted by (frame, p)
//       sort     : stable LSD radix sort on the key, 8-bit digits (per-block digit histograms, scan, per-block stable scatter):
//                  afterwards every plane's change points are contiguous and ascending
//       counts   : one thread per count slot (m + 1 counts for m change points): count r = pos[r] - pos[r-1] (pos[-1] = 0,
//                  pos[m] = H * W), its rleToString delta and character length; a scan of the lengths places the characters
//     The plan call stops there and reports per-plane count / character totals; the encode call writes counts, characters,
//     offsets, area and bbox.  Every ordered result is fixed by the data alone: the sort is stable, the scans are exact
//     integer scans, and area / bbox are integer atomics (sum, min, max) -- deterministic whatever the order of arrival.
//     The launch count depends on the key width only (<= 4 sort passes), never on F, K or the data.
// (2) Per-instance class statistics over the foreground points of all frames in one call: point counts per (frame, instance)
//     and votes of an int64 arg-max map (integer atomics), and fp64 sums of float class maps over classes 1..C-1, reduced per
//     (frame, instance) workgroup in a fixed order and then over frames in frame order (no float atomics).
#include "common.h"
#include "scan.h"

#include <algorithm>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kSortItems = 1024;         // items per workgroup in a radix pass (4 rounds of 256)

int grid_for(long long n, int cap) { return (int)std::max<long long>(1, std::min<long long>(ceil_div(n, kThreads), cap)); }

__global__ void fill_i64_kernel(long long* p, long long n, long long v) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}

// ------------------------------------------------------------------------------------------------ change points
template <typename IdxT>
__device__ __forceinline__ unsigned int map_at(const IdxT* m, long long i, int K) {
    const unsigned int v = m[i];
    return v <= (unsigned int)K ? v : 0u;            // values beyond K belong to no plane
}

// contributions of frame f, column x (one thread each; the threads of a wave read consecutive x of one row)
template <typename IdxT>
__global__ __launch_bounds__(kThreads) void rle_colcount_kernel(const IdxT* __restrict__ maps, int F, int H, int W, int K, long long* __restrict__ col_cnt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * W) return;
    const int f = (int)(i / W), x = (int)(i - (long long)f * W);
    const IdxT* m = maps + (long long)f * H * W;
    unsigned int prev = x > 0 ? map_at(m, (long long)(H - 1) * W + (x - 1), K) : 0u;
    long long c = 0;
    for (int y = 0; y < H; ++y) {
        const unsigned int v = map_at(m, (long long)y * W + x, K);
        if (v != prev) c += (prev != 0) + (v != 0);
        prev = v;
    }
    col_cnt[i] = c;
}

template <typename IdxT>
__global__ __launch_bounds__(kThreads) void rle_emit_kernel(const IdxT* __restrict__ maps, int F, int H, int W, int K, const long long* __restrict__ col_off,
                                                            long long cap, long long* __restrict__ n_eff, int* __restrict__ keys, int* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = col_off[(long long)F * W];
    if (i == 0) n_eff[0] = total <= cap ? total : 0;             // over capacity: nothing is written, the plan reports the size
    if (i >= (long long)F * W || total > cap) return;
    const int f = (int)(i / W), x = (int)(i - (long long)f * W);
    const IdxT* m = maps + (long long)f * H * W;
    unsigned int prev = x > 0 ? map_at(m, (long long)(H - 1) * W + (x - 1), K) : 0u;
    long long o = col_off[i];
    const long long o_end = col_off[i + 1];
    for (int y = 0; y < H; ++y) {
        const unsigned int v = map_at(m, (long long)y * W + x, K);
        if (v != prev) {
            const int p = x * H + y;
            if (prev != 0 && o < o_end) { keys[o] = f * K + (int)prev - 1; vals[o] = p; ++o; }
            if (v != 0 && o < o_end) { keys[o] = f * K + (int)v - 1; vals[o] = p; ++o; }
        }
        prev = v;
    }
}

// ------------------------------------------------------------------------------------------------ stable LSD radix sort
__global__ __launch_bounds__(kThreads) void radix_hist_kernel(const int* __restrict__ keys, const long long* __restrict__ n_dev, int shift, int nb,
                                                              long long* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long n = *n_dev, base = (long long)blockIdx.x * kSortItems;
    for (int r = 0; r < kSortItems / kThreads; ++r) {
        const long long i = base + r * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255], 1);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];          // digit-major: the scan orders (digit, block)
}

__global__ __launch_bounds__(kThreads) void radix_scatter_kernel(const int* __restrict__ keys, const int* __restrict__ vals, const long long* __restrict__ n_dev,
                                                                 int shift, int nb, const long long* __restrict__ hist_off, int* __restrict__ keys_out,
                                                                 int* __restrict__ vals_out) {
    __shared__ int running[256];
    __shared__ int wcnt[kThreads / 64][256];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    running[t] = 0;
    const long long n = *n_dev, base = (long long)blockIdx.x * kSortItems;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int r = 0; r < kSortItems / kThreads; ++r) {
        for (int w = 0; w < kThreads / 64; ++w) wcnt[w][t] = 0;
        __syncthreads();
        const long long i = base + r * kThreads + t;
        const bool valid = i < n;
        const int key = valid ? keys[i] : 0;
        const int d = (key >> shift) & 255;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long bb = __ballot(bit);
            same &= bit ? bb : ~bb;
        }
        if (valid && (same & lt) == 0) wcnt[wave][d] = __popcll(same);      // the lowest lane of each digit group
        __syncthreads();
        if (valid) {
            int rank = running[d] + __popcll(same & lt);
            for (int w = 0; w < wave; ++w) rank += wcnt[w][d];
            const long long o = hist_off[(long long)d * nb + blockIdx.x] + rank;
            keys_out[o] = key;
            vals_out[o] = vals[i];
        }
        __syncthreads();
        int add = 0;
        for (int w = 0; w < kThreads / 64; ++w) add += wcnt[w][t];
        running[t] += add;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ per-plane layout
__global__ void plane_hist_kernel(const int* __restrict__ keys, const long long* __restrict__ n_dev, unsigned long long* __restrict__ n_chg) {
    const long long n = *n_dev;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        atomicAdd(&n_chg[keys[i]], 1ull);
}

struct SlotInfo { long long q, r, m, begin; };

// slot index j in [0, n + P): j < n is the sorted contribution j (plane keys[j], rank j - pstart), else the last count of plane j - n
__device__ __forceinline__ SlotInfo slot_info(long long j, long long n, const int* keys, const long long* pstart) {
    SlotInfo s;
    s.q = j < n ? keys[j] : j - n;
    s.begin = pstart[s.q];
    s.m = pstart[s.q + 1] - s.begin;
    s.r = j < n ? j - s.begin : s.m;
    return s;
}

// count r of a plane: pos[r] - pos[r-1], pos[-1] = 0, pos[m] = HW
__device__ __forceinline__ long long plane_count(const int* pos, long long m, long long r, long long HW) {
    const long long hi = r < m ? pos[r] : HW, lo = r > 0 ? pos[r - 1] : 0;
    return hi - lo;
}

// rleToString: x = cnts[i] (- cnts[i-2] for i > 2), 5-bit groups LSB first, arithmetic shift, 0x20 = more, + 48
__device__ __forceinline__ int rle_chars(long long x, char* out) {
    int k = 0;
    bool more = true;
    while (more) {
        long long c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        if (out) out[k] = (char)(c + 48);
        ++k;
    }
    return k;
}

__device__ __forceinline__ long long count_delta(const int* pos, long long m, long long r, long long HW) {
    long long x = plane_count(pos, m, r, HW);
    if (r > 2) x -= plane_count(pos, m, r - 2, HW);
    return x;
}

__global__ void rle_char_len_kernel(const int* __restrict__ keys, const int* __restrict__ vals, const long long* __restrict__ n_dev, long long P,
                                    const long long* __restrict__ pstart, long long HW, long long* __restrict__ clen) {
    const long long n = *n_dev;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n + P; j += (long long)gridDim.x * blockDim.x) {
        const SlotInfo s = slot_info(j, n, keys, pstart);
        clen[s.begin + s.q + s.r] = rle_chars(count_delta(vals + s.begin, s.m, s.r, HW), nullptr);
    }
}

__global__ void rle_plan_finalize_kernel(const long long* __restrict__ n_dev, const long long* __restrict__ col_off, long long FW, long long P,
                                         const long long* __restrict__ pstart, const long long* __restrict__ coff, int* __restrict__ plane_counts,
                                         long long* __restrict__ plane_chars, long long* __restrict__ totals) {
    const long long n = *n_dev, need = col_off[FW];
    const bool ok = n == need;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < P; q += (long long)gridDim.x * blockDim.x) {
        const long long b = pstart[q] + q, e = pstart[q + 1] + q + 1;
        plane_counts[q] = ok ? (int)(e - b) : 0;
        plane_chars[q] = ok ? coff[e] - coff[b] : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals[0] = ok ? n + P : -1;
        totals[1] = ok ? coff[n + P] : -1;
        totals[2] = need;
    }
}

__global__ void rle_write_kernel(const int* __restrict__ keys, const int* __restrict__ vals, const long long* __restrict__ n_dev, long long P,
                                 const long long* __restrict__ pstart, const long long* __restrict__ coff, int H, long long HW,
                                 int* __restrict__ counts, char* __restrict__ chars, int* __restrict__ area, int* __restrict__ bb) {
    const long long n = *n_dev;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n + P; j += (long long)gridDim.x * blockDim.x) {
        const SlotInfo s = slot_info(j, n, keys, pstart);
        const int* pos = vals + s.begin;
        const long long slot = s.begin + s.q + s.r;
        counts[slot] = (int)plane_count(pos, s.m, s.r, HW);
        rle_chars(count_delta(pos, s.m, s.r, HW), chars + coff[slot]);
        if (s.r & 1) {                                       // a foreground run [pos[r-1], pos[r]) -- rleArea, rleToBbox
            const long long start = pos[s.r - 1], end = s.r < s.m ? pos[s.r] : HW;
            atomicAdd(&area[s.q], (int)(end - start));
            const int x0 = (int)(start / H), y0 = (int)(start % H), x1 = (int)((end - 1) / H), y1 = (int)((end - 1) % H);
            int* b = bb + 4 * s.q;                           // (xs, ys, xe, ye) until the finalize kernel
            atomicMin(&b[0], x0);
            atomicMax(&b[2], x1);
            if (x0 < x1) {                                   // the run crosses a column: y spans the full height
                atomicMin(&b[1], 0);
                atomicMax(&b[3], H - 1);
            } else {
                atomicMin(&b[1], min(y0, y1));
                atomicMax(&b[3], max(y0, y1));
            }
        }
    }
}

__global__ void rle_encode_init_kernel(long long P, int H, int W, int* __restrict__ area, int* __restrict__ bb) {
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < P; q += (long long)gridDim.x * blockDim.x) {
        area[q] = 0;
        bb[4 * q + 0] = W; bb[4 * q + 1] = H; bb[4 * q + 2] = 0; bb[4 * q + 3] = 0;
    }
}

__global__ void rle_encode_finalize_kernel(const long long* __restrict__ n_dev, long long P, const long long* __restrict__ pstart,
                                           const long long* __restrict__ coff, long long* __restrict__ count_offsets,
                                           long long* __restrict__ char_offsets, int* __restrict__ bb) {
    const long long n = *n_dev;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q <= P; q += (long long)gridDim.x * blockDim.x) {
        const long long b = pstart[q] + q;
        count_offsets[q] = b;
        char_offsets[q] = coff[b];
        if (q == P) continue;
        int* box = bb + 4 * q;
        if (pstart[q + 1] == pstart[q]) {                    // empty plane: counts [H*W], rleToBbox gives zeros
            box[0] = box[1] = box[2] = box[3] = 0;
        } else {
            const int xs = box[0], ys = box[1], xe = box[2], ye = box[3];
            box[0] = xs; box[1] = ys; box[2] = xe - xs + 1; box[3] = ye - ys + 1;
        }
    }
    (void)n;
}

__global__ void slot_total_kernel(long long* n_eff, long long P) { n_eff[1] = n_eff[0] + P; }

// ------------------------------------------------------------------------------------------------ workspace
struct RleWs {
    long long *col_cnt, *col_off, *tile_sums, *n_eff, *hist, *hist_off, *n_chg, *pstart, *clen, *coff;
    int *keys_a, *vals_a, *keys_b, *vals_b;
    int nb, passes;
    size_t bytes;
};

RleWs rle_layout(char* base, int F, int H, int W, int K, long long cap) {
    RleWs w;
    const long long FW = (long long)F * W, P = (long long)F * K;
    w.nb = (int)std::max<long long>(1, ceil_div(cap, kSortItems));
    long long bits = 1;
    while (bits < 31 && (1ll << bits) < P) ++bits;
    w.passes = (int)ceil_div(bits, 8);
    const long long scan_max = std::max<long long>({FW, 256ll * w.nb, P, cap + P});
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
    w.col_cnt = (long long*)take(8 * FW);
    w.col_off = (long long*)take(8 * (FW + 1));
    w.tile_sums = (long long*)take(8 * (scan_tiles(scan_max) + 1));
    w.n_eff = (long long*)take(8 * 4);
    w.hist = (long long*)take(8 * 256ll * w.nb);
    w.hist_off = (long long*)take(8 * (256ll * w.nb + 1));
    w.n_chg = (long long*)take(8 * P);
    w.pstart = (long long*)take(8 * (P + 1));
    w.clen = (long long*)take(8 * (cap + P));
    w.coff = (long long*)take(8 * (cap + P + 1));
    w.keys_a = (int*)take(4 * cap);
    w.vals_a = (int*)take(4 * cap);
    w.keys_b = (int*)take(4 * cap);
    w.vals_b = (int*)take(4 * cap);
    w.bytes = off;
    return w;
}

int check_rle_args(const void* maps, int index_bytes, int F, int H, int W, int K, long long cap, const char* who) {
    SS_CHECK_ARG(index_bytes == 1 || index_bytes == 2, "%s: index_bytes must be 1 or 2, got %d", who, index_bytes);
    SS_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && K >= 1, "%s: bad dims F=%d H=%d W=%d K=%d", who, F, H, W, K);
    SS_CHECK_ARG(K <= (index_bytes == 1 ? 255 : 65535), "%s: K=%d does not fit %d-byte indices", who, K, index_bytes);
    SS_CHECK_ARG((long long)H * W < (1ll << 31) && (long long)F * K < (1ll << 31), "%s: a plane or the plane count exceeds 2^31", who);
    SS_CHECK_ARG(cap >= 1 && cap < (1ll << 31), "%s: max_changes=%lld out of range", who, cap);
    SS_CHECK_ARG(maps != nullptr, "%s: null map", who);
    return STEMSEG_OK;
}

// ------------------------------------------------------------------------------------------------ class statistics
__device__ __forceinline__ int point_instance(long long label, const int* lut, int lut_len, int K) {
    const long long l = label + 1;
    const int v = (l >= 0 && l < lut_len) ? lut[l] : 0;
    return (v >= 1 && v <= K) ? v : 0;
}

__global__ void stats_points_kernel(const long long* __restrict__ ys, const long long* __restrict__ xs, const long long* __restrict__ labels,
                                    const long long* __restrict__ frame_off, const int* __restrict__ lut, int lut_len, int K, int h, int w,
                                    const long long* __restrict__ argmax, int C_votes, unsigned long long* __restrict__ points,
                                    unsigned long long* __restrict__ votes) {
    const int f = blockIdx.y;
    const long long b = frame_off[f], e = frame_off[f + 1];
    for (long long i = b + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (long long)gridDim.x * blockDim.x) {
        const int k = point_instance(labels[i], lut, lut_len, K);
        const long long y = ys[i], x = xs[i];
        if (k == 0 || y < 0 || y >= h || x < 0 || x >= w) continue;
        atomicAdd(&points[(long long)f * K + k - 1], 1ull);
        if (argmax) {
            const long long c = argmax[(long long)f * h * w + y * w + x];
            if (c >= 0 && c < C_votes) atomicAdd(&votes[(long long)(k - 1) * C_votes + c], 1ull);
        }
    }
}

constexpr int kClassChunk = 8;

// one workgroup per (instance k, frame f): partial[f][k-1][c-1] = sum over the frame's points of instance k of logits[f][c][y*w+x],
// c = 1..C-1; each thread sums its strided points in order, the 256 partial sums are combined by a fixed tree
__global__ __launch_bounds__(kThreads) void stats_logits_kernel(const long long* __restrict__ ys, const long long* __restrict__ xs,
                                                                const long long* __restrict__ labels, const long long* __restrict__ frame_off,
                                                                const int* __restrict__ lut, int lut_len, int K, int h, int w,
                                                                const float* __restrict__ logits, int C, double* __restrict__ partial) {
    __shared__ double sh[kClassChunk][kThreads];
    const int k = blockIdx.x + 1, f = blockIdx.y, t = threadIdx.x;
    const long long b = frame_off[f], e = frame_off[f + 1], hw = (long long)h * w;
    const float* lf = logits + (long long)f * C * hw;
    for (int c0 = 1; c0 < C; c0 += kClassChunk) {
        double acc[kClassChunk];
#pragma unroll
        for (int j = 0; j < kClassChunk; ++j) acc[j] = 0.0;
        for (long long i = b + t; i < e; i += kThreads) {
            const long long y = ys[i], x = xs[i];
            if (point_instance(labels[i], lut, lut_len, K) != k || y < 0 || y >= h || x < 0 || x >= w) continue;
            const long long pix = y * w + x;
#pragma unroll
            for (int j = 0; j < kClassChunk; ++j)
                if (c0 + j < C) acc[j] += (double)lf[(long long)(c0 + j) * hw + pix];
        }
#pragma unroll
        for (int j = 0; j < kClassChunk; ++j) sh[j][t] = acc[j];
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (t < s)
#pragma unroll
                for (int j = 0; j < kClassChunk; ++j) sh[j][t] += sh[j][t + s];
            __syncthreads();
        }
        if (t < kClassChunk && c0 + t < C) partial[((long long)f * K + (k - 1)) * (C - 1) + (c0 + t - 1)] = sh[t][0];
        __syncthreads();
    }
}

__global__ void stats_reduce_frames_kernel(const double* __restrict__ partial, int F, long long KC, double* __restrict__ sums) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < KC; i += (long long)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int f = 0; f < F; ++f) s += partial[(long long)f * KC + i];
        sums[i] = s;
    }
}

}  // namespace

extern "C" size_t stemseg_hip_rle_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t K, int64_t max_changes) {
    if (F < 1 || H < 1 || W < 1 || K < 1 || max_changes < 1) return 0;
    return rle_layout(nullptr, F, H, W, K, max_changes).bytes;
}

extern "C" int stemseg_hip_rle_plan(const void* maps, int32_t index_bytes, int32_t F, int32_t H, int32_t W, int32_t K, int64_t max_changes,
                                    void* workspace, size_t ws_bytes, int32_t* plane_counts, int64_t* plane_chars, int64_t* totals, void* stream) {
    int rc = check_rle_args(maps, index_bytes, F, H, W, K, max_changes, "rle_plan");
    if (rc != STEMSEG_OK) return rc;
    SS_CHECK_ARG(workspace && plane_counts && plane_chars && totals, "rle_plan: null pointer");
    RleWs w = rle_layout(static_cast<char*>(workspace), F, H, W, K, max_changes);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "rle_plan: workspace %zu bytes < %zu", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const long long FW = (long long)F * W, P = (long long)F * K, cap = max_changes, HW = (long long)H * W;
    if (index_bytes == 1) {
        hipLaunchKernelGGL(rle_colcount_kernel<unsigned char>, dim3(ceil_div(FW, kThreads)), dim3(kThreads), 0, s, static_cast<const unsigned char*>(maps), F, H, W, K, w.col_cnt);
    } else {
        hipLaunchKernelGGL(rle_colcount_kernel<unsigned short>, dim3(ceil_div(FW, kThreads)), dim3(kThreads), 0, s, static_cast<const unsigned short*>(maps), F, H, W, K, w.col_cnt);
    }
    launch_scan(w.col_cnt, nullptr, FW, w.tile_sums, w.col_off, s);
    if (index_bytes == 1) {
        hipLaunchKernelGGL(rle_emit_kernel<unsigned char>, dim3(ceil_div(FW, kThreads)), dim3(kThreads), 0, s, static_cast<const unsigned char*>(maps), F, H, W, K,
                           w.col_off, cap, w.n_eff, w.keys_a, w.vals_a);
    } else {
        hipLaunchKernelGGL(rle_emit_kernel<unsigned short>, dim3(ceil_div(FW, kThreads)), dim3(kThreads), 0, s, static_cast<const unsigned short*>(maps), F, H, W, K,
                           w.col_off, cap, w.n_eff, w.keys_a, w.vals_a);
    }
    int *kin = w.keys_a, *vin = w.vals_a, *kout = w.keys_b, *vout = w.vals_b;
    for (int pass = 0; pass < w.passes; ++pass) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3(w.nb), dim3(kThreads), 0, s, kin, w.n_eff, 8 * pass, w.nb, w.hist);
        launch_scan(w.hist, nullptr, 256ll * w.nb, w.tile_sums, w.hist_off, s);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(w.nb), dim3(kThreads), 0, s, kin, vin, w.n_eff, 8 * pass, w.nb, w.hist_off, kout, vout);
        std::swap(kin, kout);
        std::swap(vin, vout);
    }
    if (kin != w.keys_a) {                   // the sorted list always ends in (keys_a, vals_a): the encode call reads it there
        SS_HIP(hipMemcpyAsync(w.keys_a, kin, 4 * cap, hipMemcpyDeviceToDevice, s));
        SS_HIP(hipMemcpyAsync(w.vals_a, vin, 4 * cap, hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(fill_i64_kernel, dim3(grid_for(P, 1024)), dim3(kThreads), 0, s, w.n_chg, P, 0ll);
    hipLaunchKernelGGL(plane_hist_kernel, dim3(grid_for(cap, 4096)), dim3(kThreads), 0, s, w.keys_a, w.n_eff, reinterpret_cast<unsigned long long*>(w.n_chg));
    launch_scan(w.n_chg, nullptr, P, w.tile_sums, w.pstart, s);
    hipLaunchKernelGGL(rle_char_len_kernel, dim3(grid_for(cap + P, 4096)), dim3(kThreads), 0, s, w.keys_a, w.vals_a, w.n_eff, P, w.pstart, HW, w.clen);
    hipLaunchKernelGGL(slot_total_kernel, dim3(1), dim3(1), 0, s, w.n_eff, P);      // the scan length n + P is device-side
    launch_scan(w.clen, w.n_eff + 1, cap + P, w.tile_sums, w.coff, s);
    hipLaunchKernelGGL(rle_plan_finalize_kernel, dim3(grid_for(P, 1024)), dim3(kThreads), 0, s, w.n_eff, w.col_off, FW, P, w.pstart, w.coff,
                       plane_counts, reinterpret_cast<long long*>(plane_chars), reinterpret_cast<long long*>(totals));
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_rle_encode(const void* maps, int32_t index_bytes, int32_t F, int32_t H, int32_t W, int32_t K, int64_t max_changes,
                                      void* workspace, size_t ws_bytes, int32_t* counts, int64_t* count_offsets, uint8_t* chars,
                                      int64_t* char_offsets, int32_t* area, int32_t* bbox, void* stream) {
    int rc = check_rle_args(maps, index_bytes, F, H, W, K, max_changes, "rle_encode");
    if (rc != STEMSEG_OK) return rc;
    SS_CHECK_ARG(workspace && counts && count_offsets && chars && char_offsets && area && bbox, "rle_encode: null pointer");
    RleWs w = rle_layout(static_cast<char*>(workspace), F, H, W, K, max_changes);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "rle_encode: workspace %zu bytes < %zu", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const long long P = (long long)F * K, cap = max_changes, HW = (long long)H * W;
    hipLaunchKernelGGL(rle_encode_init_kernel, dim3(grid_for(P, 1024)), dim3(kThreads), 0, s, P, H, W, area, bbox);
    hipLaunchKernelGGL(rle_write_kernel, dim3(grid_for(cap + P, 4096)), dim3(kThreads), 0, s, w.keys_a, w.vals_a, w.n_eff, P, w.pstart, w.coff, H, HW,
                       counts, reinterpret_cast<char*>(chars), area, bbox);
    hipLaunchKernelGGL(rle_encode_finalize_kernel, dim3(grid_for(P + 1, 1024)), dim3(kThreads), 0, s, w.n_eff, P, w.pstart, w.coff,
                       reinterpret_cast<long long*>(count_offsets), reinterpret_cast<long long*>(char_offsets), bbox);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_instance_class_stats(const int64_t* ys, const int64_t* xs, const int64_t* labels, const int64_t* frame_offsets, int32_t F,
                                                int64_t max_frame_points, const int32_t* lut, int32_t lut_len, int32_t K, int32_t h, int32_t w,
                                                const float* logits, int32_t C_logits, double* partial, double* sums, const int64_t* argmax,
                                                int32_t C_votes, int64_t* points, int64_t* votes, void* stream) {
    SS_CHECK_ARG(F >= 1 && K >= 1 && h >= 1 && w >= 1 && lut_len >= 0 && max_frame_points >= 0, "instance_class_stats: bad dims F=%d K=%d h=%d w=%d", F, K, h, w);
    SS_CHECK_ARG(frame_offsets && points && (max_frame_points == 0 || (ys && xs && labels && lut)), "instance_class_stats: null pointer");
    SS_CHECK_ARG(!logits || (C_logits >= 2 && partial && sums), "instance_class_stats: logits need C >= 2 and partial / sums buffers");
    SS_CHECK_ARG(!argmax || (C_votes >= 1 && votes), "instance_class_stats: argmax needs C_votes >= 1 and a votes buffer");
    SS_CHECK_ARG(F <= 65535, "instance_class_stats: F=%d frames exceed one launch", F);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(fill_i64_kernel, dim3(grid_for((long long)F * K, 1024)), dim3(kThreads), 0, s, reinterpret_cast<long long*>(points), (long long)F * K, 0ll);
    if (argmax)
        hipLaunchKernelGGL(fill_i64_kernel, dim3(grid_for((long long)K * C_votes, 1024)), dim3(kThreads), 0, s, reinterpret_cast<long long*>(votes),
                           (long long)K * C_votes, 0ll);
    if (max_frame_points > 0)
        hipLaunchKernelGGL(stats_points_kernel, dim3(grid_for(max_frame_points, 256), F), dim3(kThreads), 0, s, reinterpret_cast<const long long*>(ys),
                           reinterpret_cast<const long long*>(xs), reinterpret_cast<const long long*>(labels), reinterpret_cast<const long long*>(frame_offsets),
                           lut, lut_len, K, h, w, reinterpret_cast<const long long*>(argmax), C_votes, reinterpret_cast<unsigned long long*>(points),
                           reinterpret_cast<unsigned long long*>(votes));
    if (logits) {
        if (max_frame_points > 0) {
            hipLaunchKernelGGL(stats_logits_kernel, dim3(K, F), dim3(kThreads), 0, s, reinterpret_cast<const long long*>(ys), reinterpret_cast<const long long*>(xs),
                               reinterpret_cast<const long long*>(labels), reinterpret_cast<const long long*>(frame_offsets), lut, lut_len, K, h, w, logits,
                               C_logits, partial);
        } else {
            hipLaunchKernelGGL(fill_i64_kernel, dim3(grid_for((long long)F * K * (C_logits - 1), 1024)), dim3(kThreads), 0, s,
                               reinterpret_cast<long long*>(partial), (long long)F * K * (C_logits - 1), 0ll);
        }
        hipLaunchKernelGGL(stats_reduce_frames_kernel, dim3(grid_for((long long)K * (C_logits - 1), 1024)), dim3(kThreads), 0, s, partial, F,
                           (long long)K * (C_logits - 1), sums);
    }
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
