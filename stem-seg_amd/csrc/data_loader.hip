// Device half of the training data loader (data/video_dataset.py, generic_video_dataset_parser.py:74-94, structures/mask.py:32-40).
//
// (1) rle_decode: the inverse of writers.hip -- M concatenated COCO RLE strings -> binary planes, pycocotools' rleFrString + rleDecode
//     (characters are 48 + a 6-bit group, 0x20 = more follows, the last group sign-extended from 0x10, count i > 2 a delta against
//     count i - 2, runs alternate from zeros, column-major p = x * H + y).  Every table is indexed by CHARACTER position, the entry of
//     a count sitting at its last character and every other entry being zero, so nothing is compacted and no length is read back:
//       mark     : one thread per character: is it a group end, is it outside 48..111 (both in one int64: ends low, bad high)
//       scan     : cs = exclusive scan -> the count index of a character, and per string the number of bad characters
//       assemble : the thread at a count's last character gathers its <= 12 groups into the delta x, and files it under its parity
//                  chain (even counts from 2 on | odd counts), two sections of one array
//       scan     : one scan over both sections; a count is its chain's inclusive sum minus the sum at the string's first character
//       counts   : count -> (count | out of range), two sections of one array
//       scan     : run starts, and per string the sum of the counts and the number of counts out of range
//       status   : one thread per string: the first check that fails, or 0
//       raster   : one thread per pixel of every plane: the string of its plane, then a binary search for the last character whose
//                  run start is <= p; the run's parity is the value.  Planes no string names, and planes of refused strings, are 0.
//     Integer arithmetic only, no atomics, every output fixed by the data; 16 launches whatever M, P or the data.
//     Malformed strings cannot move a write: the only stores into `planes` are the rasteriser's, at the thread's own pixel index.
// (1b) rle_decode_union: the same strings, but a plane is the OR of every accepted string that names it (the Mapillary ignore mask: a
//     hundred segments of a 9 MP image in ONE plane, no plane per segment).  mark .. status are rle_decode's, unchanged; then
//       tables   : one thread per plane: its strings [first, last) (the plane indices do not decrease, so two binary searches); one
//                  thread per string: the interval [p_lo, p_hi) of column-major pixels outside which it holds no foreground -- its
//                  first count, and H * W minus its last count when that closes a zero run; empty for a refused string.  A zero-length
//                  run inside only leaves the interval wider than it need be, never narrower.
//       raster   : one thread per pixel of every plane: it walks the strings of its plane (the range and each string's interval are
//                  uniform over the workgroup and come through scalar loads), searches those whose interval holds its p, stops at
//                  the first hit.
//     15 launches whatever M, P or the data; the same rules: integers, no atomics, one store per thread at its own pixel index.
// (1c) rle_decode_labels: the same strings and the same tables as (1b), but every string carries a label 1 .. 65535 and a plane is a
//     uint16 LABEL MAP: the largest label among the accepted strings of the plane that are 1 at the pixel, else 0 (the KITTI-MOTS
//     evaluation: the masks of one frame in ONE map, no plane per mask), and per plane the number of pixels that more than one accepted
//     string covers.  mark .. status and tables are unchanged; then
//       fill     : overlap[0 .. P) = 0
//       raster   : one thread per pixel of every plane: it walks ALL the strings of its plane whose interval holds its p (no early
//                  stop: the second hit is what `overlap` counts), keeps the largest label, stores it at its own pixel; the threads'
//                  overlap flags are summed over the wave, then over the workgroup in LDS, and one integer atomic per workgroup and
//                  plane (none when the sum is 0) adds them to overlap[plane].  Sums of ones: the same bits in every run.
//     16 launches whatever M, P or the data; integers only, no copy, no synchronisation.
// (1d) rle_pair_inter: the same strings and the same parse, but NO plane: per string its number of 1-pixels, and per (string, string)
//     pair of a list the number of pixels that are 1 in both, computed on the runs (the YouTube-VIS evaluation: the track IoU needs the
//     intersection of every result mask with every ground-truth mask of its frame).  mark .. status are unchanged; then
//       area     : a workgroup per string: the sum of its odd counts, and its extent by (1b)'s rule
//       pairs    : a workgroup per pair, its threads over the characters of the longer string: the thread at the end of an odd count
//                  owns that run's pixel interval, searches the other string for the run that covers its start ((1)'s search) and
//                  walks forward adding the overlap with the odd runs until one starts past its end.  Disjoint extents end a pair at once.
//     Sums through shuffles and LDS, stored once by thread 0: no atomics.  15 launches whatever M, the pairs or the data; the workspace
//     holds the string tables and one extent per string, nothing per pixel.
//     What (1) .. (1d) share is written once: on the device covering_char and is_one_run (the search and the parity of its hit),
//     column_major (a pixel's p), string_extent ((1b)'s interval) and block_sum_int (the workgroup sums of (1c) and (1d)); on the host
//     check_sizes, check_offsets and check_plane_order (the argument checks, in the one order every entry point reports them in) and
//     parse_strings (the workspace check, then mark .. status).
// (2) resize_masks: planes -> bilinear(new size, align_corners=False) > 0.5 -> zero pad, torch's formula in unfused fp32 (bilinear.h), and
//     optional extra output planes computed from 1 - any(planes[range]) taken at full resolution before the resize
//     (davis_data_loader.py:86-88).
#include "common.h"
#include "bilinear.h"
#include "scan.h"

#include <algorithm>
#include <climits>
#include <vector>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGroups = 12;                    // 60 bits: the sign extension shifts by at most 60
constexpr long long kBadX = LLONG_MIN;
constexpr long long kLow32 = 0xffffffffll;
constexpr long long kMaxChars = 1ll << 30;

int grid_for(long long n, int cap) { return (int)std::max<long long>(1, std::min<long long>(ceil_div(n, kThreads), cap)); }

__device__ __forceinline__ bool char_valid(unsigned char c) { return c >= 48 && c <= 111; }
__device__ __forceinline__ bool char_is_end(unsigned char c) { return char_valid(c) && !((c - 48) & 0x20); }

// largest m with offs[m] <= i, for 0 <= i < offs[M] (empty strings are skipped: their range holds no i)
__device__ __forceinline__ int string_of_char(const long long* __restrict__ offs, int M, long long i) {
    int lo = 0, hi = M;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void plane_table_fill_kernel(int* __restrict__ sop, int P) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x) sop[q] = -1;
}

// (the host has checked that the plane indices are distinct and below P)
__global__ void plane_table_kernel(const int* __restrict__ plane_of_string, int M, int P, int* __restrict__ sop) {
    for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
        const int q = plane_of_string[m];
        if (q >= 0 && q < P) sop[q] = m;
    }
}

__global__ void rle_mark_kernel(const unsigned char* __restrict__ chars, long long N, long long* __restrict__ flag) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const unsigned char c = chars[i];
        flag[i] = (char_is_end(c) ? 1ll : 0ll) + (char_valid(c) ? 0ll : (1ll << 32));
    }
}

// X[i]: the delta of the count that ends at character i (kBadX: more than kMaxGroups groups, a bad character among them, or a value
// no plane below 2^31 pixels can hold); chain[i] / chain[N + i]: the same under the even (local index >= 2) / odd chain
__global__ void rle_assemble_kernel(const unsigned char* __restrict__ chars, long long N, const long long* __restrict__ offs, int M,
                                    const long long* __restrict__ cs, long long* __restrict__ X, long long* __restrict__ chain) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        long long x = 0, xe = 0, xo = 0;
        if (char_is_end(chars[i])) {
            const long long lo = offs[string_of_char(offs, M, i)];
            const int r = (int)(cs[i] & kLow32) - (int)(cs[lo] & kLow32);
            long long first = i;
            while (first > lo && i - first < kMaxGroups - 1 && !char_is_end(chars[first - 1])) --first;
            bool bad = first > lo && !char_is_end(chars[first - 1]);
            const int n = (int)(i - first) + 1;
            unsigned long long u = 0;
            for (int k = 0; k < n; ++k) {
                const unsigned char c = chars[first + k];
                bad = bad || !char_valid(c);
                u |= (unsigned long long)((c - 48) & 0x1f) << (5 * k);
            }
            if ((chars[i] - 48) & 0x10) u |= ~0ull << (5 * n);
            x = (long long)u;
            bad = bad || x > (1ll << 31) || x < -(1ll << 31);
            if (bad) {
                x = kBadX;
            } else if (r & 1) {
                xo = x;
            } else if (r >= 2) {
                xe = x;
            }
        }
        X[i] = x;
        chain[i] = xe;
        chain[N + i] = xo;
    }
}

__global__ void rle_counts_kernel(const unsigned char* __restrict__ chars, long long N, const long long* __restrict__ offs, int M,
                                  const long long* __restrict__ cs, const long long* __restrict__ X, const long long* __restrict__ chain_sum,
                                  long long HW, long long* __restrict__ cnt) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        long long c = 0, bad = 0;
        if (char_is_end(chars[i])) {
            const long long lo = offs[string_of_char(offs, M, i)];
            const int r = (int)(cs[i] & kLow32) - (int)(cs[lo] & kLow32);
            const long long x = X[i];
            if (x == kBadX) {
                bad = 1;
            } else {
                c = r == 0 ? x : (r & 1) ? chain_sum[N + i + 1] - chain_sum[N + lo] : chain_sum[i + 1] - chain_sum[lo];
                if (c < 0 || c > HW) { bad = 1; c = 0; }
            }
        }
        cnt[i] = c;
        cnt[N + i] = bad;
    }
}

__global__ void rle_status_kernel(const unsigned char* __restrict__ chars, long long N, const long long* __restrict__ offs, int M,
                                  const long long* __restrict__ cs, const long long* __restrict__ cnt_sum, long long HW,
                                  unsigned char* __restrict__ status) {
    for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
        const long long lo = offs[m], hi = offs[m + 1];
        unsigned char st = 0;
        if (hi == lo) st = STEMSEG_RLE_EMPTY;
        else if ((cs[hi] >> 32) != (cs[lo] >> 32)) st = STEMSEG_RLE_BAD_CHAR;
        else if (!char_is_end(chars[hi - 1])) st = STEMSEG_RLE_OPEN_GROUP;
        else if (cnt_sum[N + hi] != cnt_sum[N + lo]) st = STEMSEG_RLE_BAD_COUNT;
        else if (cnt_sum[hi] - cnt_sum[lo] != HW) st = STEMSEG_RLE_BAD_SUM;
        status[m] = st;
    }
}

// The covering run: the last character of [lo, hi) whose run start cnt_sum[i] - base is <= p (base = cnt_sum at the string's first
// character).  For an accepted string the counts are >= 0 and sum to HW > p, so that character ends a count that is > 0 and covers p.
__device__ __forceinline__ long long covering_char(const long long* __restrict__ cnt_sum, long long base, long long lo, long long hi, long long p) {
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (cnt_sum[mid] - base <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// is the run of the count that ends at character i a 1-run: its count index (first = that of the string's first character) is odd
__device__ __forceinline__ bool is_one_run(const long long* __restrict__ cs, long long first, long long i) { return ((cs[i] & kLow32) - first) & 1; }

// pixel i of a row-major H x W plane -> its column-major index p = x * H + y (H * W < 2^31)
__device__ __forceinline__ unsigned int column_major(unsigned int i, int H, int W) {
    const unsigned int y = i / (unsigned int)W, x = i - y * (unsigned int)W;
    return x * (unsigned int)H + y;
}

// [p_lo, p_hi) of the accepted string [lo, hi) (lo < hi, every character valid, the last one ends a count, every count in [0, HW]): every
// foreground pixel p = x * H + y lies inside -- its first count is a zero run; with an odd number of counts so is its last.  All-zero
// string: one count of H * W, so [H * W, 0) is empty; all-one string: counts 0, H * W, so [0, H * W).
__device__ __forceinline__ int2 string_extent(const unsigned char* __restrict__ chars, const long long* __restrict__ cs,
                                              const long long* __restrict__ cnt, long long lo, long long hi, long long HW) {
    long long first_end = lo;
    while (first_end < hi - 1 && !char_is_end(chars[first_end])) ++first_end;
    const int n_counts = (int)(cs[hi] & kLow32) - (int)(cs[lo] & kLow32);
    return make_int2((int)cnt[first_end], (int)((n_counts & 1) ? HW - cnt[hi - 1] : HW));
}

// the workgroup's sum of v, in every thread (shuffles inside a wave, four words of LDS across the waves); met by every thread
__device__ __forceinline__ int block_sum_int(int v, int* wave_sums) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();                                                                   // the previous sum has been read
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    int total = 0;
    for (int k = 0; k < kThreads / 64; ++k) total += wave_sums[k];
    return total;
}

// One thread per pixel: the value is the parity of the covering run's count index.
__global__ __launch_bounds__(kThreads) void rle_raster_kernel(const int* __restrict__ sop, const unsigned char* __restrict__ status,
                                                              const long long* __restrict__ offs, const long long* __restrict__ cs,
                                                              const long long* __restrict__ cnt_sum, int P, int H, int W,
                                                              unsigned char* __restrict__ planes) {
    // planes along grid y, pixels along grid x: H * W < 2^31, so a pixel's index and its divisions are 32-bit, and what depends on the
    // plane alone is read once per plane
    const unsigned int HW = (unsigned int)H * (unsigned int)W;
    for (int q = blockIdx.y; q < P; q += gridDim.y) {
        const int m = sop[q];
        const bool live = m >= 0 && status[m] == 0;
        const long long first_char = live ? offs[m] : 0, end_char = live ? offs[m + 1] : 0;
        const long long base = live ? cnt_sum[first_char] : 0, first = live ? (cs[first_char] & kLow32) : 0;
        unsigned char* plane = planes + (long long)q * HW;
        for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
            plane[i] = live && is_one_run(cs, first, covering_char(cnt_sum, base, first_char, end_char, column_major(i, H, W)));
        }
    }
}

// ---- rle_decode_union: a plane is the OR of its strings
// first m with plane_of_string[m] >= q (the host has checked that the plane indices do not decrease)
__device__ __forceinline__ int first_string_of_plane(const int* __restrict__ plane_of_string, int M, int q) {
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (plane_of_string[mid] < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// range[q] = the strings [first, last) of plane q; extent[m] = string_extent of an accepted string, empty for a refused one
__global__ void union_tables_kernel(const int* __restrict__ plane_of_string, int M, int P, const unsigned char* __restrict__ status,
                                    const unsigned char* __restrict__ chars, const long long* __restrict__ offs,
                                    const long long* __restrict__ cs, const long long* __restrict__ cnt, long long HW,
                                    int2* __restrict__ range, int2* __restrict__ extent) {
    const int n = M > P ? M : P;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i < P) range[i] = make_int2(first_string_of_plane(plane_of_string, M, i), first_string_of_plane(plane_of_string, M, i + 1));
        if (i < M) extent[i] = status[i] == 0 ? string_extent(chars, cs, cnt, offs[i], offs[i + 1], HW) : make_int2(0, 0);
    }
}

// One thread per pixel, as rle_raster_kernel; the search is the same, once per string whose extent holds p, until one says 1.
__global__ __launch_bounds__(kThreads) void rle_raster_union_kernel(const int2* __restrict__ range, const int2* __restrict__ extent,
                                                                    const long long* __restrict__ offs, const long long* __restrict__ cs,
                                                                    const long long* __restrict__ cnt_sum, int P, int H, int W,
                                                                    unsigned char* __restrict__ planes) {
    const unsigned int HW = (unsigned int)H * (unsigned int)W;
    for (int q = blockIdx.y; q < P; q += gridDim.y) {
        const int2 strings = range[q];
        unsigned char* plane = planes + (long long)q * HW;
        for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
            const int p = (int)column_major(i, H, W);
            unsigned char v = 0;
            for (int m = strings.x; m < strings.y; ++m) {
                const int2 e = extent[m];
                if (v == 0 && p >= e.x && p < e.y) {
                    const long long first_char = offs[m];
                    v = is_one_run(cs, cs[first_char] & kLow32, covering_char(cnt_sum, cnt_sum[first_char], first_char, offs[m + 1], p));
                }
            }
            plane[i] = v;
        }
    }
}

// ---- rle_decode_labels: a plane is a label map
__global__ void overlap_fill_kernel(int* __restrict__ overlap, int P) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x) overlap[q] = 0;
}

// One thread per pixel, as rle_raster_union_kernel, but every string whose extent holds p is searched: the largest label of those that
// say 1 is the value, and a pixel with two or more of them counts once in overlap[q].  The plane loop is uniform over the workgroup,
// so the barriers of the reduction are met by every thread.
__global__ __launch_bounds__(kThreads) void rle_raster_labels_kernel(const int2* __restrict__ range, const int2* __restrict__ extent,
                                                                     const int* __restrict__ label_of_string,
                                                                     const long long* __restrict__ offs, const long long* __restrict__ cs,
                                                                     const long long* __restrict__ cnt_sum, int P, int H, int W,
                                                                     unsigned short* __restrict__ maps, int* __restrict__ overlap) {
    __shared__ int wave_sums[kThreads / 64];
    const unsigned int HW = (unsigned int)H * (unsigned int)W;
    for (int q = blockIdx.y; q < P; q += gridDim.y) {
        const int2 strings = range[q];
        unsigned short* plane = maps + (long long)q * HW;
        int doubles = 0;
        for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
            const int p = (int)column_major(i, H, W);
            int best = 0, hits = 0;
            for (int m = strings.x; m < strings.y; ++m) {
                const int2 e = extent[m];
                if (p >= e.x && p < e.y) {
                    const long long first_char = offs[m];
                    if (is_one_run(cs, cs[first_char] & kLow32, covering_char(cnt_sum, cnt_sum[first_char], first_char, offs[m + 1], p))) {
                        const int label = label_of_string[m];
                        best = label > best ? label : best;
                        ++hits;
                    }
                }
            }
            plane[i] = (unsigned short)best;
            doubles += hits > 1 ? 1 : 0;
        }
        doubles = block_sum_int(doubles, wave_sums);          // (its first barrier: the previous plane's sum has been read)
        if (threadIdx.x == 0 && doubles) atomicAdd(&overlap[q], doubles);
    }
}

// ---- rle_pair_inter: the intersection of two parsed strings, on their runs
// A workgroup per string, striding over the strings: area[m] = the sum of its odd counts (one thread per character; the entry of a count
// sits at its last character, every other entry is 0), extent[m] = its string_extent.  Both 0 / empty for a refused string.
__global__ __launch_bounds__(kThreads) void rle_area_kernel(int M, const unsigned char* __restrict__ status, const unsigned char* __restrict__ chars,
                                                            const long long* __restrict__ offs, const long long* __restrict__ cs,
                                                            const long long* __restrict__ cnt, long long HW, int* __restrict__ area,
                                                            int2* __restrict__ extent) {
    __shared__ int wave_sums[kThreads / 64];
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const bool live = status[m] == 0;
        const long long lo = live ? offs[m] : 0, hi = live ? offs[m + 1] : 0;
        const int first = live ? (int)(cs[lo] & kLow32) : 0;
        int sum = 0;
        for (long long i = lo + threadIdx.x; i < hi; i += kThreads)
            if (is_one_run(cs, first, i)) sum += (int)cnt[i];
        sum = block_sum_int(sum, wave_sums);
        if (threadIdx.x == 0) {
            area[m] = sum;
            extent[m] = live ? string_extent(chars, cs, cnt, lo, hi, HW) : make_int2(0, 0);
        }
    }
}

// A workgroup per pair, striding over the pairs.  Its threads stride over the characters of the pair's LONGER string (the intersection
// is symmetric; the longer side has the more runs to share out).  A thread whose character ends an odd, non-empty count owns the pixel
// interval [s, e) of that run, clipped to the other string's extent; it searches the other string's characters for the last one with run
// start <= s (covering_char: that character ends the count that covers s) and walks forward, a character at a time, adding
// the overlap of the odd counts until one starts at or after e.  A character that ends no count has a zero entry and adds nothing.  The
// walk stays inside [lo, hi) of the other string whatever the tables hold; inter[k] is stored once, by thread 0.
__global__ __launch_bounds__(kThreads) void rle_pair_inter_kernel(const int* __restrict__ pairs, int n_pairs, int M,
                                                                  const unsigned char* __restrict__ status, const int2* __restrict__ extent,
                                                                  const long long* __restrict__ offs, const long long* __restrict__ cs,
                                                                  const long long* __restrict__ cnt, const long long* __restrict__ cnt_sum,
                                                                  int* __restrict__ inter) {
    __shared__ int wave_sums[kThreads / 64];
    for (int k = blockIdx.x; k < n_pairs; k += gridDim.x) {
        int2 pr = make_int2(pairs[2 * k], pairs[2 * k + 1]);
        bool live = pr.x >= 0 && pr.x < M && pr.y >= 0 && pr.y < M;
        live = live && status[pr.x] == 0 && status[pr.y] == 0;
        int sum = 0;
        if (live) {
            if (offs[pr.y + 1] - offs[pr.y] > offs[pr.x + 1] - offs[pr.x]) pr = make_int2(pr.y, pr.x);
            const int2 ea = extent[pr.x], eb = extent[pr.y];
            if (ea.x < eb.y && eb.x < ea.y) {                                          // (an empty extent fails one of the two)
                const long long alo = offs[pr.x], ahi = offs[pr.x + 1], blo = offs[pr.y], bhi = offs[pr.y + 1];
                const long long abase = cnt_sum[alo], bbase = cnt_sum[blo];
                const int afirst = (int)(cs[alo] & kLow32), bfirst = (int)(cs[blo] & kLow32);
                for (long long i = alo + threadIdx.x; i < ahi; i += kThreads) {
                    const long long len = cnt[i];
                    if (len <= 0 || !is_one_run(cs, afirst, i)) continue;
                    long long s = cnt_sum[i] - abase, e = s + len;
                    s = s > eb.x ? s : eb.x;
                    e = e < eb.y ? e : eb.y;
                    if (s >= e) continue;
                    const long long lo = covering_char(cnt_sum, bbase, blo, bhi, s);
                    long long start = cnt_sum[lo] - bbase;
                    for (long long j = lo; j < bhi && start < e; ++j) {
                        const long long end = cnt_sum[j + 1] - bbase;
                        if (is_one_run(cs, bfirst, j)) {
                            const long long a0 = start > s ? start : s, a1 = end < e ? end : e;
                            if (a1 > a0) sum += (int)(a1 - a0);
                        }
                        start = end;
                    }
                }
            }
        }
        sum = block_sum_int(sum, wave_sums);
        if (threadIdx.x == 0) inter[k] = sum;
    }
}

struct DecodeWs {
    long long *flag, *cs, *tile_sums, *X, *chain, *chain_sum, *cnt, *cnt_sum;
    int* sop;
    int2 *range, *extent;          // rle_decode_union and rle_decode_labels alone
    size_t bytes;
};

DecodeWs decode_layout(char* base, long long n_chars, int M, int P, bool is_union) {
    DecodeWs w;
    const long long N = std::max<long long>(n_chars, 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
    w.sop = nullptr;
    w.range = w.extent = nullptr;
    if (is_union) {
        w.range = (int2*)take(8 * (size_t)std::max(P, 1));
        w.extent = (int2*)take(8 * (size_t)std::max(M, 1));
    } else {
        w.sop = (int*)take(4 * (size_t)std::max(P, 1));
    }
    w.flag = (long long*)take(8 * N);
    w.cs = (long long*)take(8 * (N + 1));
    w.tile_sums = (long long*)take(8 * ((size_t)scan_tiles(2 * N) + 1));
    w.X = (long long*)take(8 * N);
    w.chain = (long long*)take(16 * N);
    w.chain_sum = (long long*)take(8 * (2 * N + 1));
    w.cnt = (long long*)take(16 * N);
    w.cnt_sum = (long long*)take(8 * (2 * N + 1));
    w.bytes = off;
    return w;
}

struct UnionRanges {
    int n;
    int start[STEMSEG_MAX_UNION_RANGES], count[STEMSEG_MAX_UNION_RANGES], stride[STEMSEG_MAX_UNION_RANGES];
};

__device__ __forceinline__ float plane_value(const unsigned char* __restrict__ planes, long long HW0, long long pix, int q, int P,
                                             const UnionRanges& ur) {
    if (q < P) return planes[(long long)q * HW0 + pix] ? 1.f : 0.f;
    const int r = q - P;
    bool any = false;
    for (int k = 0; k < ur.count[r]; ++k) any = any || planes[(long long)(ur.start[r] + k * ur.stride[r]) * HW0 + pix];
    return any ? 0.f : 1.f;
}

// one thread per pixel of the padded output; the source pixel is mirrored in x under flip_x
__global__ __launch_bounds__(kThreads) void resize_masks_kernel(const unsigned char* __restrict__ planes, int P, int H0, int W0, int nh, int nw,
                                                                int PH, int PW, float sy, float sx, int flip_x, UnionRanges ur,
                                                                unsigned char* __restrict__ out) {
    const long long plane = (long long)PH * PW, n = (long long)(P + ur.n) * plane, HW0 = (long long)H0 * W0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i / plane);
        const long long r = i - (long long)q * plane;
        const int y = (int)(r / PW), x = (int)(r - (long long)y * PW);
        unsigned char v = 0;
        if (y < nh && x < nw) {
            const Tap ty = make_tap(sy, y, H0), tx = make_tap(sx, x, W0);
            const int x0 = flip_x ? W0 - 1 - tx.i0 : tx.i0, x1 = flip_x ? W0 - 1 - tx.i1 : tx.i1;
            const float v00 = plane_value(planes, HW0, (long long)ty.i0 * W0 + x0, q, P, ur);
            const float v01 = plane_value(planes, HW0, (long long)ty.i0 * W0 + x1, q, P, ur);
            const float v10 = plane_value(planes, HW0, (long long)ty.i1 * W0 + x0, q, P, ur);
            const float v11 = plane_value(planes, HW0, (long long)ty.i1 * W0 + x1, q, P, ur);
            v = lerp2(v00, v01, v10, v11, ty, tx) > 0.5f ? 1 : 0;
        }
        out[i] = v;
    }
}

// ---- what the four entry points share on the host.  The order of the checks is part of the ABI: the first rule broken is the one reported.
// The dimensions (`second` names the fourth: P >= 1 planes, or n_pairs >= 0), rle_decode's plane for every string, the 2^31 plane, the
// characters, the entry point's null pointers
int check_sizes(const char* who, int M, const char* second, int P, int min_P, int H, int W, bool plane_each, long long n_chars, bool non_null) {
    SS_CHECK_ARG(M >= 0 && P >= min_P && H >= 1 && W >= 1, "%s: bad dims M=%d %s=%d H=%d W=%d", who, M, second, P, H, W);
    SS_CHECK_ARG(!plane_each || P >= M, "%s: %d strings for %d planes", who, M, P);
    SS_CHECK_ARG((long long)H * W < (1ll << 31), "%s: a plane of %d x %d exceeds 2^31 pixels", who, H, W);
    SS_CHECK_ARG(n_chars >= 0 && n_chars < kMaxChars, "%s: n_chars=%lld out of range", who, n_chars);
    SS_CHECK_ARG(non_null, "%s: null pointer", who);
    return STEMSEG_OK;
}

// The ends of the offsets, then string by string: its offsets, then what the entry point asks of that string (per_string(m) -> a status)
template <class PerString>
int check_offsets(const char* who, const int64_t* offsets_host, int M, long long n_chars, PerString per_string) {
    SS_CHECK_ARG(offsets_host[0] == 0 && offsets_host[M] == n_chars, "%s: offsets must run from 0 to n_chars=%lld", who, n_chars);
    for (int m = 0; m < M; ++m) {
        SS_CHECK_ARG(offsets_host[m + 1] >= offsets_host[m], "%s: offsets decrease at string %d", who, m);
        if (const int rc = per_string(m)) return rc;
    }
    return STEMSEG_OK;
}

// rle_decode_union and rle_decode_labels: string m names a plane below P, and none before the plane of string m - 1
int check_plane_order(const char* who, const int32_t* plane_of_string_host, int m, int P) {
    const int q = plane_of_string_host[m];
    SS_CHECK_ARG(q >= 0 && q < P, "%s: string %d names plane %d of %d", who, m, q, P);
    SS_CHECK_ARG(m == 0 || q >= plane_of_string_host[m - 1], "%s: the plane indices decrease at string %d (%d after %d)", who, m, q,
                 m ? plane_of_string_host[m - 1] : 0);
    return STEMSEG_OK;
}

struct Parsed { DecodeWs w; hipStream_t s; long long HW; const long long* offs; };          // what the kernels after the parse are given

// The workspace laid out and checked -- the last check -- then mark .. status: everything that does not depend on the planes (13 launches)
int parse_strings(const char* who, void* workspace, size_t ws_bytes, const uint8_t* chars, long long N, const int64_t* offsets, int M, int P,
                  bool is_union, int H, int W, uint8_t* status, void* stream, Parsed* out) {
    const DecodeWs w = decode_layout(static_cast<char*>(workspace), N, M, P, is_union);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "%s: workspace %zu bytes < %zu", who, ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const long long HW = (long long)H * W;
    const long long* offs = reinterpret_cast<const long long*>(offsets);
    *out = Parsed{w, s, HW, offs};
    hipLaunchKernelGGL(rle_mark_kernel, dim3(grid_for(N, 4096)), dim3(kThreads), 0, s, chars, N, w.flag);
    launch_scan(w.flag, nullptr, N, w.tile_sums, w.cs, s);
    hipLaunchKernelGGL(rle_assemble_kernel, dim3(grid_for(N, 4096)), dim3(kThreads), 0, s, chars, N, offs, M, w.cs, w.X, w.chain);
    launch_scan(w.chain, nullptr, 2 * N, w.tile_sums, w.chain_sum, s);
    hipLaunchKernelGGL(rle_counts_kernel, dim3(grid_for(N, 4096)), dim3(kThreads), 0, s, chars, N, offs, M, w.cs, w.X, w.chain_sum, HW, w.cnt);
    launch_scan(w.cnt, nullptr, 2 * N, w.tile_sums, w.cnt_sum, s);
    hipLaunchKernelGGL(rle_status_kernel, dim3(grid_for(M, 1024)), dim3(kThreads), 0, s, chars, N, offs, M, w.cs, w.cnt_sum, HW, status);
    return STEMSEG_OK;
}

}  // namespace

extern "C" size_t stemseg_hip_rle_decode_workspace_bytes(int64_t n_chars, int32_t M, int32_t P) {
    if (n_chars < 0 || n_chars >= kMaxChars || M < 0 || P < 1) return 0;
    return decode_layout(nullptr, n_chars, M, P, false).bytes;
}

extern "C" int stemseg_hip_rle_decode(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* plane_of_string_host,
                                      const int64_t* offsets, const int32_t* plane_of_string, int32_t M, int32_t P, int32_t H, int32_t W,
                                      void* workspace, size_t ws_bytes, uint8_t* planes, uint8_t* status, void* stream) {
    const char* who = "rle_decode";
    const bool non_null = planes && workspace && offsets_host && offsets && (M == 0 || (plane_of_string_host && plane_of_string && status)) &&
                          (n_chars == 0 || chars);
    if (const int rc = check_sizes(who, M, "P", P, 1, H, W, true, n_chars, non_null)) return rc;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(offsets) % 8 == 0 && reinterpret_cast<uintptr_t>(plane_of_string) % 4 == 0,
                 "rle_decode: the device offsets must be 8-byte aligned, the device plane indices 4-byte aligned");
    std::vector<char> named((size_t)P, 0);
    const auto distinct_plane = [&](int m) -> int {
        const int q = plane_of_string_host[m];
        SS_CHECK_ARG(q >= 0 && q < P, "rle_decode: string %d names plane %d of %d", m, q, P);
        SS_CHECK_ARG(!named[q], "rle_decode: plane %d is named by two strings", q);
        named[q] = 1;
        return STEMSEG_OK;
    };
    Parsed t;
    if (const int rc = check_offsets(who, offsets_host, M, n_chars, distinct_plane)) return rc;
    if (const int rc = parse_strings(who, workspace, ws_bytes, chars, n_chars, offsets, M, P, false, H, W, status, stream, &t)) return rc;
    hipLaunchKernelGGL(plane_table_fill_kernel, dim3(grid_for(P, 1024)), dim3(kThreads), 0, t.s, t.w.sop, P);
    hipLaunchKernelGGL(plane_table_kernel, dim3(grid_for(M, 1024)), dim3(kThreads), 0, t.s, plane_of_string, M, P, t.w.sop);
    hipLaunchKernelGGL(rle_raster_kernel, dim3(grid_for(t.HW, 1024), std::min(P, 1024)), dim3(kThreads), 0, t.s, t.w.sop, status, t.offs, t.w.cs,
                       t.w.cnt_sum, P, H, W, planes);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_rle_decode_union_workspace_bytes(int64_t n_chars, int32_t M, int32_t P) {
    if (n_chars < 0 || n_chars >= kMaxChars || M < 0 || P < 1) return 0;
    return decode_layout(nullptr, n_chars, M, P, true).bytes;
}

extern "C" int stemseg_hip_rle_decode_union(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* plane_of_string_host,
                                            const int64_t* offsets, const int32_t* plane_of_string, int32_t M, int32_t P, int32_t H, int32_t W,
                                            void* workspace, size_t ws_bytes, uint8_t* planes, uint8_t* status, void* stream) {
    const char* who = "rle_decode_union";
    const bool non_null = planes && workspace && offsets_host && offsets && (M == 0 || (plane_of_string_host && plane_of_string && status)) &&
                          (n_chars == 0 || chars);
    if (const int rc = check_sizes(who, M, "P", P, 1, H, W, false, n_chars, non_null)) return rc;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(offsets) % 8 == 0 && reinterpret_cast<uintptr_t>(plane_of_string) % 4 == 0,
                 "rle_decode_union: the device offsets must be 8-byte aligned, the device plane indices 4-byte aligned");
    const auto plane_order = [&](int m) { return check_plane_order(who, plane_of_string_host, m, P); };
    Parsed t;
    if (const int rc = check_offsets(who, offsets_host, M, n_chars, plane_order)) return rc;
    if (const int rc = parse_strings(who, workspace, ws_bytes, chars, n_chars, offsets, M, P, true, H, W, status, stream, &t)) return rc;
    hipLaunchKernelGGL(union_tables_kernel, dim3(grid_for(std::max(M, P), 1024)), dim3(kThreads), 0, t.s, plane_of_string, M, P, status, chars,
                       t.offs, t.w.cs, t.w.cnt, t.HW, t.w.range, t.w.extent);
    hipLaunchKernelGGL(rle_raster_union_kernel, dim3(grid_for(t.HW, 1024), std::min(P, 1024)), dim3(kThreads), 0, t.s, t.w.range, t.w.extent, t.offs,
                       t.w.cs, t.w.cnt_sum, P, H, W, planes);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_rle_decode_labels_workspace_bytes(int64_t n_chars, int32_t M, int32_t P) {
    return stemseg_hip_rle_decode_union_workspace_bytes(n_chars, M, P);          // the same tables
}

extern "C" int stemseg_hip_rle_decode_labels(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* plane_of_string_host,
                                             const int32_t* label_of_string_host, const int64_t* offsets, const int32_t* plane_of_string,
                                             const int32_t* label_of_string, int32_t M, int32_t P, int32_t H, int32_t W, void* workspace,
                                             size_t ws_bytes, uint16_t* maps, int32_t* overlap, uint8_t* status, void* stream) {
    const char* who = "rle_decode_labels";
    const bool non_null = maps && overlap && workspace && offsets_host && offsets &&
                          (M == 0 || (plane_of_string_host && plane_of_string && label_of_string_host && label_of_string && status)) &&
                          (n_chars == 0 || chars);
    if (const int rc = check_sizes(who, M, "P", P, 1, H, W, false, n_chars, non_null)) return rc;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(offsets) % 8 == 0 && reinterpret_cast<uintptr_t>(plane_of_string) % 4 == 0 &&
                 reinterpret_cast<uintptr_t>(label_of_string) % 4 == 0,
                 "rle_decode_labels: the device offsets must be 8-byte aligned, the device plane indices and labels 4-byte aligned");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(maps) % 2 == 0 && reinterpret_cast<uintptr_t>(overlap) % 4 == 0,
                 "rle_decode_labels: misaligned maps (uint16) or overlap (int32)");
    const auto plane_and_label = [&](int m) -> int {
        if (const int rc = check_plane_order(who, plane_of_string_host, m, P)) return rc;
        const int label = label_of_string_host[m];
        SS_CHECK_ARG(label >= 1 && label <= 65535, "rle_decode_labels: string %d has label %d, outside 1 .. 65535", m, label);
        return STEMSEG_OK;
    };
    Parsed t;
    if (const int rc = check_offsets(who, offsets_host, M, n_chars, plane_and_label)) return rc;
    if (const int rc = parse_strings(who, workspace, ws_bytes, chars, n_chars, offsets, M, P, true, H, W, status, stream, &t)) return rc;
    hipLaunchKernelGGL(union_tables_kernel, dim3(grid_for(std::max(M, P), 1024)), dim3(kThreads), 0, t.s, plane_of_string, M, P, status, chars,
                       t.offs, t.w.cs, t.w.cnt, t.HW, t.w.range, t.w.extent);
    hipLaunchKernelGGL(overlap_fill_kernel, dim3(grid_for(P, 1024)), dim3(kThreads), 0, t.s, overlap, P);
    hipLaunchKernelGGL(rle_raster_labels_kernel, dim3(grid_for(t.HW, 1024), std::min(P, 1024)), dim3(kThreads), 0, t.s, t.w.range, t.w.extent,
                       label_of_string, t.offs, t.w.cs, t.w.cnt_sum, P, H, W, maps, overlap);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_rle_pair_inter_workspace_bytes(int64_t n_chars, int32_t M, int32_t n_pairs) {
    if (n_chars < 0 || n_chars >= kMaxChars || M < 0 || n_pairs < 0) return 0;
    return decode_layout(nullptr, n_chars, M, 1, true).bytes;          // the string tables and one extent per string: nothing per pixel
}

extern "C" int stemseg_hip_rle_pair_inter(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* pairs_host,
                                          const int64_t* offsets, const int32_t* pairs, int32_t M, int32_t n_pairs, int32_t H, int32_t W,
                                          void* workspace, size_t ws_bytes, int32_t* area, int32_t* inter, uint8_t* status, void* stream) {
    const char* who = "rle_pair_inter";
    const bool non_null = workspace && offsets_host && offsets && (M == 0 || (area && status)) && (n_pairs == 0 || (pairs_host && pairs && inter)) &&
                          (n_chars == 0 || chars);
    if (const int rc = check_sizes(who, M, "n_pairs", n_pairs, 0, H, W, false, n_chars, non_null)) return rc;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(offsets) % 8 == 0, "rle_pair_inter: the device offsets must be 8-byte aligned");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(pairs) % 4 == 0 && reinterpret_cast<uintptr_t>(area) % 4 == 0 &&
                 reinterpret_cast<uintptr_t>(inter) % 4 == 0, "rle_pair_inter: misaligned pairs, area or inter (int32)");
    if (const int rc = check_offsets(who, offsets_host, M, n_chars, [](int) { return STEMSEG_OK; })) return rc;
    for (int k = 0; k < n_pairs; ++k)
        SS_CHECK_ARG(pairs_host[2 * k] >= 0 && pairs_host[2 * k] < M && pairs_host[2 * k + 1] >= 0 && pairs_host[2 * k + 1] < M,
                     "rle_pair_inter: pair %d names strings (%d, %d) of %d", k, pairs_host[2 * k], pairs_host[2 * k + 1], M);
    Parsed t;
    if (const int rc = parse_strings(who, workspace, ws_bytes, chars, n_chars, offsets, M, 1, true, H, W, status, stream, &t)) return rc;
    hipLaunchKernelGGL(rle_area_kernel, dim3(std::max(1, std::min(M, 4096))), dim3(kThreads), 0, t.s, M, status, chars, t.offs, t.w.cs, t.w.cnt, t.HW,
                       area, t.w.extent);
    hipLaunchKernelGGL(rle_pair_inter_kernel, dim3(std::max(1, std::min(n_pairs, 8192))), dim3(kThreads), 0, t.s,
                       pairs, n_pairs, M, status, t.w.extent, t.offs, t.w.cs, t.w.cnt, t.w.cnt_sum, inter);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_resize_masks(const uint8_t* planes, int32_t P, int32_t H0, int32_t W0, int32_t new_h, int32_t new_w, int32_t pad_h,
                                        int32_t pad_w, const int32_t* union_ranges_host, int32_t n_ranges, int32_t flip_x, uint8_t* out,
                                        void* stream) {
    SS_CHECK_ARG(planes && out, "resize_masks: null pointer");
    SS_CHECK_ARG(P >= 1 && H0 >= 1 && W0 >= 1 && new_h >= 1 && new_w >= 1 && pad_h >= new_h && pad_w >= new_w,
                 "resize_masks: bad dims %d x (%d, %d) -> (%d, %d) padded (%d, %d)", P, H0, W0, new_h, new_w, pad_h, pad_w);
    SS_CHECK_ARG((long long)H0 * W0 < (1ll << 31) && (long long)pad_h * pad_w < (1ll << 31), "resize_masks: a plane exceeds 2^31 pixels");
    SS_CHECK_ARG(n_ranges >= 0 && n_ranges <= STEMSEG_MAX_UNION_RANGES && (n_ranges == 0 || union_ranges_host),
                 "resize_masks: %d union ranges (at most %d)", n_ranges, STEMSEG_MAX_UNION_RANGES);
    UnionRanges ur;
    ur.n = n_ranges;
    for (int r = 0; r < STEMSEG_MAX_UNION_RANGES; ++r) ur.start[r] = ur.count[r] = ur.stride[r] = 0;
    for (int r = 0; r < n_ranges; ++r) {
        const int start = union_ranges_host[3 * r], count = union_ranges_host[3 * r + 1], stride = union_ranges_host[3 * r + 2];
        SS_CHECK_ARG(start >= 0 && count >= 1 && stride >= 1 && (long long)start + (long long)(count - 1) * stride < P,
                     "resize_masks: union range %d (start %d, count %d, stride %d) leaves the %d planes", r, start, count, stride, P);
        ur.start[r] = start; ur.count[r] = count; ur.stride[r] = stride;
    }
    const float sy = (float)H0 / (float)new_h, sx = (float)W0 / (float)new_w;       // size-driven bilinear: scale = in / out
    hipLaunchKernelGGL(resize_masks_kernel, dim3(grid_for((long long)(P + n_ranges) * pad_h * pad_w, 1 << 16)), dim3(kThreads), 0, as_stream(stream),
                       planes, P, H0, W0, new_h, new_w, pad_h, pad_w, sy, sx, flip_x ? 1 : 0, ur, out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
