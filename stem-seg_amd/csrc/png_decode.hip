// PNG decoder for 8-bit, non-interlaced gray / RGB / gray+alpha / RGBA files, pixel-identical to libpng (cv2.imread IMREAD_COLOR)
// and PIL's convert("RGB").  F frames of one geometry (size, channels) per call; each frame is its IDAT payloads concatenated into
// one zlib stream (stemseg_amd/utils/png.py walks the chunks).  Stages, a fixed launch count whatever the data:
//   init     : per frame, the header blob against the call's geometry and the stream offsets
//   crc      : one wave per IDAT chunk: each lane a table CRC-32 of its piece, the pieces joined with the GF(2) shift operator
//              (zlib's crc32_combine algebra: crc(A||B) = crc(A) * x^(8|B|) mod P ^ crc(B)), then the chunk type in front
//   finder   : one thread per 64 bit positions of the streams tests each for a dynamic-Huffman block header (BTYPE 10, HLIT <= 286,
//              HDIST <= 30, a complete code-length code, literal/length and distance lengths that decode without overrun or a
//              leading repeat, both codes complete under zlib's rule, a nonzero EOB length); the exact scan (scan.h) over the
//              per-word counts compacts the candidates in bit order
//   spec     : one wave per candidate decodes its block speculatively from the header: lane 0 builds the tables in LDS, then the
//              wave decodes the body with self-synchronising subsequences of sub_bits bits (wave_body): end bit, output length,
//              validity (literal/length symbols 286 / 287 and distance symbols 30 / 31 are invalid)
//   chain    : one thread per frame checks the zlib header (CM 8, CINFO <= 7, FCHECK, no FDICT) and walks the blocks from the
//              first: a dynamic block at a valid candidate takes the candidate's end, anything else -- a stored or fixed block, a
//              missed candidate -- is decoded by the serial backstop; the running output offset gives every block its place.
//              A missing final block, BTYPE 11, a stored length mismatch, bytes after the Adler-32 or an inflated length other
//              than H * (1 + W * channels) is corruption
//   write    : one wave per confirmed block (a scan of the per-frame block counts lists them) decodes it again from its exact
//              start, each lane its settled subsequence at its prefix-sum place: a literal writes its byte, a copied byte
//              the index of its source (dst - dist + (i mod dist), so overlapping copies point before the copy); a distance
//              before the start of the stream is corruption
//   frame    : one workgroup per frame resolves every source index by pointer jumping until each points at a literal (the
//              round count depends on the data, the loop stays inside the workgroup), gathers the bytes, checks the Adler-32 and
//              the filter types (<= 4), unfilters as a diagonal wavefront (lane = row, each row one pixel behind the row above,
//              since Sub / Avg / Paeth need the pixel to the left) and writes BGR (gray replicated, alpha dropped)
// Status per frame: bit 0 corrupt (the pixels are undefined; the caller decodes the file on the host); bit 1 a block's
// synchronisation took more than one round; bit 2 the serial backstop decoded at least one block.
#include "common.h"
#include "scan.h"

#include <algorithm>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kTabThreads = 64;               // the finder and the chain keep a Huffman table pair per thread in LDS
constexpr int kFrameThreads = 1024;
constexpr int kHdrWords = 8;
constexpr long long kMaxStream = 1ll << 28;   // frame-local bit positions stay in int32 range
constexpr unsigned int kCrcPoly = 0xEDB88320u;
constexpr int kMinBlockBits = 10;             // the smallest DEFLATE block: a fixed block holding only EOB
constexpr int kDefaultSubBits = 512;
constexpr int kWaveGrid = 8192;               // workgroups of the grid-stride wave kernels

enum : int { kCorrupt = 1, kMultiRound = 2, kBackstop = 4 };
enum : int { kNoFinder = 1 };

__host__ __device__ __forceinline__ long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
__host__ __device__ __forceinline__ long long rup(long long a, long long b) { return cdiv(a, b) * b; }
__host__ __device__ __forceinline__ long long lmax(long long a, long long b) { return a > b ? a : b; }

struct Geo {
    int F, H, W, C, flags, sub_bits;
    long long raw;                            // inflated bytes per frame: H * (1 + W * C)
    long long total_bytes;
    long long NW;                             // 64-bit words of candidate mask
    long long NCmax;                          // candidate slots
    long long NB;                             // block slots
    long long NCH;                            // IDAT record bound
};

struct Ws {
    int* flags;               // [F]
    long long* nblk;          // [F] confirmed blocks
    long long* bscan;         // [F + 1]
    unsigned long long* mask; // [NW] candidate bits
    long long* wcnt;          // [NW]
    long long* woff;          // [NW + 1]
    long long* cand;          // [NCmax] global bit position of a candidate
    long long* cend;          // [NCmax] global end bit, -1 if the block is invalid
    long long* colen;         // [NCmax] output bytes
    long long* bstart;        // [NB] frame-local start bit of a confirmed block
    long long* boff;          // [NB] its frame-local output offset
    int* src;                 // [F * raw] literal: -1 - byte; copy: frame-local index of the source byte
    unsigned char* px;        // [F * raw] inflated, then unfiltered bytes
    long long* tile_sums;
    size_t bytes;
};

Ws layout(char* base, const Geo& g) {
    Ws w{};
    size_t o = 0;
    auto take = [&](long long n) { void* p = base ? base + o : nullptr; o += rup(lmax(n, 1), 256); return p; };
    w.flags = (int*)take(4 * g.F);
    w.nblk = (long long*)take(8 * g.F);
    w.bscan = (long long*)take(8 * (g.F + 1));
    w.mask = (unsigned long long*)take(8 * g.NW);
    w.wcnt = (long long*)take(8 * g.NW);
    w.woff = (long long*)take(8 * (g.NW + 1));
    w.cand = (long long*)take(8 * g.NCmax);
    w.cend = (long long*)take(8 * g.NCmax);
    w.colen = (long long*)take(8 * g.NCmax);
    w.bstart = (long long*)take(8 * g.NB);
    w.boff = (long long*)take(8 * g.NB);
    w.src = (int*)take(4 * g.F * g.raw);
    w.px = (unsigned char*)take(g.F * g.raw);
    w.tile_sums = (long long*)take(8 * (scan_tiles(std::max<long long>(g.NW, g.F)) + 1));
    w.bytes = o;
    return w;
}

int grid(long long n, int threads = kThreads) { return (int)std::max<long long>(1, cdiv(n, threads)); }

// ------------------------------------------------------------------------------------------------ frame lookup
// the frame holding stream byte b: the last f with offsets[f] <= b (empty frames are skipped by taking the last)
__device__ int frame_of_byte(const long long* __restrict__ offsets, int F, long long b) {
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ long long slot_base(const long long* __restrict__ offsets, int f) { return offsets[f] * 8 / kMinBlockBits + f; }

// ------------------------------------------------------------------------------------------------ bit reader
// A frame's stream: bytes s[0, n).  Bits are read LSB first; bytes past n read as 0 (the caller checks the end position).
struct Bits {
    const unsigned char* s;
    long long n;
    __device__ __forceinline__ unsigned int byte(long long i) const { return i < n ? s[i] : 0u; }
    __device__ __forceinline__ unsigned int peek(long long pos) const {          // 32 bits from bit pos (pos >= 0)
        const long long b = pos >> 3;
        const unsigned long long v = (unsigned long long)byte(b) | ((unsigned long long)byte(b + 1) << 8) | ((unsigned long long)byte(b + 2) << 16) |
                                     ((unsigned long long)byte(b + 3) << 24) | ((unsigned long long)byte(b + 4) << 32);
        return (unsigned int)(v >> (pos & 7));
    }
    __device__ __forceinline__ unsigned int get(long long& pos, int k) const {   // k <= 24
        const unsigned int v = peek(pos) & ((1u << k) - 1u);
        pos += k;
        return v;
    }
};

// ------------------------------------------------------------------------------------------------ Huffman codes (puff style)
struct Lit { short count[16]; short sym[288]; };
struct Dist { short count[16]; short sym[32]; };
struct Tabs {                                // one thread's tables and header scratch, in LDS
    Lit lit;
    Dist dist;
    short ccount[16], csym[20], offs[16];
    unsigned char len[320];
};

// canonical code of lengths[0..n): returns the Kraft remainder (0 complete, > 0 incomplete, < 0 over-subscribed); *maxlen the
// longest length
__device__ int build(short* count, short* sym, short* offs, const unsigned char* lengths, int n, int* maxlen) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) count[lengths[i]]++;
    int left = 1, mx = 0;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= count[l];
        if (count[l]) mx = l;
        if (left < 0) { *maxlen = mx; return left; }
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + count[l];
    for (int i = 0; i < n; ++i)
        if (lengths[i]) sym[offs[lengths[i]]++] = (short)i;
    *maxlen = mx;
    return left;
}

// one symbol from the 32 bits at pos; -1 if the bits are no code of the table (an incomplete code's hole)
__device__ __forceinline__ int decode(const short* count, const short* sym, const Bits& bs, long long& pos) {
    const unsigned int v = bs.peek(pos);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (v >> (l - 1)) & 1u;
        const int c = count[l];
        if (code - c < first) {
            pos += l;
            return sym[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// zlib's rule: over-subscribed is invalid; incomplete only for a code whose longest length is 1
__device__ __forceinline__ bool code_ok(int left, int maxlen) { return left == 0 || (left > 0 && maxlen == 1); }

// The dynamic header at pos (after BFINAL / BTYPE): builds t and advances pos; false if zlib would reject it.
__device__ bool dynamic_header(const Bits& bs, long long& pos, long long end, Tabs& t) {
    constexpr unsigned char kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    unsigned char* len = t.len;
    const int nlen = (int)bs.get(pos, 5) + 257, ndist = (int)bs.get(pos, 5) + 1, ncode = (int)bs.get(pos, 4) + 4;
    if (nlen > 286 || ndist > 30) return false;
    for (int i = 0; i < 19; ++i) len[kOrder[i]] = i < ncode ? (unsigned char)bs.get(pos, 3) : 0;
    if (pos > end) return false;
    int mx;
    if (build(t.ccount, t.csym, t.offs, len, 19, &mx) != 0) return false;          // the code-length code must be complete
    int i = 0;
    while (i < nlen + ndist) {
        const int s = decode(t.ccount, t.csym, bs, pos);
        if (s < 0 || pos > end) return false;
        if (s < 16) {
            len[i++] = (unsigned char)s;
            continue;
        }
        int rep, val = 0;
        if (s == 16) {
            if (i == 0) return false;                                   // a repeat with nothing before it
            val = len[i - 1];
            rep = 3 + (int)bs.get(pos, 2);
        } else if (s == 17) {
            rep = 3 + (int)bs.get(pos, 3);
        } else {
            rep = 11 + (int)bs.get(pos, 7);
        }
        if (i + rep > nlen + ndist || pos > end) return false;
        while (rep--) len[i++] = (unsigned char)val;
    }
    if (len[256] == 0) return false;                                   // no end-of-block code
    int lm, dm;
    const int ll = build(t.lit.count, t.lit.sym, t.offs, len, nlen, &lm);
    if (!code_ok(ll, lm)) return false;
    const int dl = build(t.dist.count, t.dist.sym, t.offs, len + nlen, ndist, &dm);
    return dm == 0 || code_ok(dl, dm);                                  // no distance codes at all is allowed
}

__device__ void fixed_tables(Tabs& t) {
    unsigned char* len = t.len;
    int mx;
    for (int i = 0; i < 288; ++i) len[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    build(t.lit.count, t.lit.sym, t.offs, len, 288, &mx);
    for (int i = 0; i < 30; ++i) len[i] = 5;
    len[30] = len[31] = 5;
    build(t.dist.count, t.dist.sym, t.offs, len, 32, &mx);
}

__constant__ short kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ unsigned char kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ int kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                  4097, 6145, 8193, 12289, 16385, 24577};
__constant__ unsigned char kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

// The Huffman-coded body of a block from pos (after its header) to its EOB.  Counting mode (src == nullptr): *olen gets the
// output length.  A distance beyond the window is rejected (zlib may reject it, depending on how it is called).  Writing mode: literals and source indices go to src[o0 ..]; a distance before the stream's start is corruption.
// Returns false on an invalid code, a length or distance symbol out of range, an overrun of the stream, or more output than
// `cap` bytes (o0 + output).
__device__ bool huffman_body(const Bits& bs, long long& pos, long long end, const Tabs& t, long long o0, long long cap, int window, int* src,
                             long long* olen) {
    long long o = o0;
    for (;;) {
        const int s = decode(t.lit.count, t.lit.sym, bs, pos);
        if (s < 0 || pos > end) return false;
        if (s < 256) {
            if (o >= cap) return false;
            if (src) src[o] = -1 - s;
            ++o;
            continue;
        }
        if (s == 256) break;
        if (s > 285) return false;
        const int li = s - 257;
        const int n = kLenBase[li] + (int)bs.get(pos, kLenExtra[li]);
        const int ds = decode(t.dist.count, t.dist.sym, bs, pos);
        if (ds < 0 || ds > 29) return false;
        const int d = kDistBase[ds] + (int)bs.get(pos, kDistExtra[ds]);
        if (pos > end || o + n > cap || d > window) return false;
        if (src) {
            if (o - d < 0) return false;
            for (int i = 0; i < n; ++i) src[o + i] = (int)(o - d + (i % d));
        }
        o += n;
    }
    *olen = o - o0;
    return true;
}

// One whole block from its header at pos.  Returns false if zlib would reject it; else pos is its end, *final its BFINAL.
__device__ bool block(const Bits& bs, long long& pos, long long end, Tabs& t, long long o0, long long cap, int* src, long long* olen, int* final) {
    const int window = 1 << ((bs.byte(0) >> 4) + 8);                  // CINFO: zlib rejects a distance beyond the window
    *final = (int)bs.get(pos, 1);
    const int type = (int)bs.get(pos, 2);
    if (type == 0) {
        pos = (pos + 7) & ~7ll;
        const unsigned int ln = bs.get(pos, 16), nl = bs.get(pos, 16);
        if ((ln ^ 0xFFFFu) != nl || pos + 8ll * ln > end || o0 + ln > cap) return false;
        if (src)
            for (unsigned int i = 0; i < ln; ++i) src[o0 + i] = -1 - (int)bs.byte((pos >> 3) + i);
        pos += 8ll * ln;
        *olen = ln;
        return true;
    }
    if (type == 3) return false;
    if (type == 1) fixed_tables(t);
    else if (!dynamic_header(bs, pos, end, t)) return false;
    return huffman_body(bs, pos, end, t, o0, cap, window, src, olen);
}

// ------------------------------------------------------------------------------------------------ wave decode of a block body
// One subsequence: tokens from pos while pos < stop (a token that starts before stop is decoded whole).  Returns 0 when it reached
// stop (pos is then the first token start at or past it), 1 at the block's EOB (pos just after it), 2 on an invalid code, an
// overrun, more than cap output bytes or a distance beyond the window.  *cnt: output bytes.  Writing mode (src): the bytes go to
// src[o ..] and a distance before the stream's start is invalid too.
__device__ int sub_walk(const Bits& bs, long long& pos, long long stop, long long end, const Tabs& t, int window, long long o, long long cap, int* src,
                        long long* cnt) {
    long long c = 0;
    int code = 0;
    while (pos < stop) {
        const int s = decode(t.lit.count, t.lit.sym, bs, pos);
        if (s < 0 || pos > end) { code = 2; break; }
        if (s < 256) {
            if (o + c >= cap) { code = 2; break; }
            if (src) src[o + c] = -1 - s;
            ++c;
            continue;
        }
        if (s == 256) { code = 1; break; }
        if (s > 285) { code = 2; break; }
        const int li = s - 257;
        const int n = kLenBase[li] + (int)bs.get(pos, kLenExtra[li]);
        const int ds = decode(t.dist.count, t.dist.sym, bs, pos);
        if (ds < 0 || ds > 29) { code = 2; break; }
        const int d = kDistBase[ds] + (int)bs.get(pos, kDistExtra[ds]);
        if (pos > end || o + c + n > cap || d > window) { code = 2; break; }
        if (src) {
            if (o + c - d < 0) { code = 2; break; }
            for (int i = 0; i < n; ++i) src[o + c + i] = (int)(o + c - d + (i % d));
        }
        c += n;
    }
    *cnt = c;
    return code;
}

// A Huffman block body from `start` (after its header) decoded by the whole wave with self-synchronising subsequences of sub_bits
// bits, in windows of 64: lane k of a window starts speculatively at base + k * sub_bits; then, in rounds, every lane whose
// predecessor's exit differs from its input re-decodes from that exit, until no input changes (lane 0's input is exact, so round r
// settles lane r at the latest).  A lane after one that met the EOB or an invalid code is past the block.  The next window starts
// at lane 63's exit.  Writing mode: once a window has settled, each lane decodes its subsequence again into src at its place (a
// prefix sum of the counts).  Every lane of the wave calls this; *end, *olen and the return value are the same in every lane.
// *multi: some window needed more than one round.
__device__ bool wave_body(const Bits& bs, long long start, long long end, const Tabs& t, int window, long long o0, long long cap, int* src,
                          int sub_bits, long long* end_pos, long long* olen, bool* multi) {
    const int lane = threadIdx.x & 63;
    long long base = start, out = o0;
    for (;;) {
        const long long stop = base + (long long)(lane + 1) * sub_bits;
        long long in = base + (long long)lane * sub_bits, p = in, cnt = 0;
        bool alive = in < end;
        int code = 3;                                                   // 3: past the block
        if (alive) code = sub_walk(bs, p, stop, end, t, window, 0, cap, nullptr, &cnt);
        int rounds = 0;
        for (;;) {
            const long long pe = __shfl_up(p, 1, 64);
            const int pc = __shfl_up(code, 1, 64);
            bool change = false;
            if (lane > 0) {
                if (pc == 0) {
                    if (!alive || pe != in) {
                        alive = true;
                        in = p = pe;
                        code = sub_walk(bs, p, stop, end, t, window, 0, cap, nullptr, &cnt);
                        change = true;
                    }
                } else if (alive) {
                    alive = false;
                    code = 3;
                    cnt = 0;
                    change = true;
                }
            }
            if (!__any(change)) break;
            ++rounds;
        }
        if (rounds > 1) *multi = true;
        // the first lane that did not reach its stop ends the block (EOB) or makes it invalid
        const unsigned long long ended = __ballot(code != 0);
        const int last = ended ? __ffsll((long long)ended) - 1 : 63;
        const int last_code = __shfl(code, last, 64);
        if (last_code >= 2) return false;
        long long pre = lane <= last ? cnt : 0;                         // inclusive prefix sum of the counts
        for (int k = 1; k < 64; k <<= 1) {
            const long long v = __shfl_up(pre, k, 64);
            if (lane >= k) pre += v;
        }
        const long long total = __shfl(pre, 63, 64);
        if (out + total > cap) return false;
        if (src) {
            int bad = 0;
            if (lane <= last) {
                long long q = in, c2;
                bad = sub_walk(bs, q, stop, end, t, window, out + pre - cnt, cap, src, &c2) >= 2;
            }
            if (__any(bad)) return false;
        }
        out += total;
        const long long exit = __shfl(p, last, 64);
        if (ended) {
            *end_pos = exit;
            *olen = out - o0;
            return true;
        }
        base = exit;
    }
}

struct FrameView {
    Bits bs;
    long long bits;
};

__device__ __forceinline__ FrameView frame_view(const unsigned char* data, const long long* offsets, int f) {
    FrameView v;
    v.bs.s = data + offsets[f];
    v.bs.n = offsets[f + 1] - offsets[f];
    v.bits = v.bs.n * 8;
    return v;
}

// ------------------------------------------------------------------------------------------------ init
__global__ void init_kernel(Geo g, const long long* __restrict__ offsets, const long long* __restrict__ hdr, int* __restrict__ flags) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= g.F) return;
    const long long* h = hdr + (long long)f * kHdrWords;
    const long long len = offsets[f + 1] - offsets[f];
    const bool ok = h[0] == g.H && h[1] == g.W && h[2] == g.C && h[3] == len && len >= 0 && len < kMaxStream && offsets[f + 1] <= g.total_bytes &&
                    h[4] >= 0 && h[5] >= 1 && h[4] + h[5] <= g.NCH;
    flags[f] = ok ? 0 : kCorrupt;
}

// ------------------------------------------------------------------------------------------------ CRC-32 of the IDAT chunks
__device__ unsigned int multmodp(unsigned int a, unsigned int b) {   // a * b mod P, reflected (zlib crc32.c)
    unsigned int m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

__device__ unsigned int x8nmodp(long long n, const unsigned int* x2n) {   // x^(8n) mod P
    unsigned int p = 1u << 31;
    int k = 3;
    while (n) {
        if (n & 1) p = multmodp(x2n[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
}

__global__ __launch_bounds__(kThreads) void crc_kernel(Geo g, const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                       const long long* __restrict__ hdr, const unsigned int* __restrict__ recs, int* __restrict__ flags) {
    __shared__ unsigned int tab[256];
    __shared__ unsigned int x2n[32];
    const int t = threadIdx.x, lane = t & 63;
    {
        unsigned int c = t;
        for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ kCrcPoly : c >> 1;
        tab[t] = c;
    }
    if (t == 0) {
        unsigned int p = 1u << 30;                                       // x^1
        x2n[0] = p;
        for (int n = 1; n < 32; ++n) x2n[n] = p = multmodp(p, p);
    }
    __syncthreads();
    const long long* last = hdr + (long long)(g.F - 1) * kHdrWords;
    const long long n_rec = min(g.NCH, last[4] + last[5]);
    const long long waves = (long long)gridDim.x * (kThreads / 64);
    for (long long r = (long long)blockIdx.x * (kThreads / 64) + (t >> 6); r < n_rec; r += waves) {
        const unsigned int off = recs[4 * r], len = recs[4 * r + 1], stored = recs[4 * r + 2], f = recs[4 * r + 3];
        if (f >= (unsigned int)g.F) continue;
        const long long flen = offsets[f + 1] - offsets[f];
        if ((long long)off + len > flen) {
            if (lane == 0) atomicOr(&flags[f], kCorrupt);
            continue;
        }
        const unsigned char* p = data + offsets[f] + off;
        const long long pl = cdiv(len, 64);
        const long long b = min((long long)len, lane * pl), e = min((long long)len, b + pl);
        unsigned int c = 0xFFFFFFFFu;
        for (long long i = b; i < e; ++i) c = tab[(c ^ p[i]) & 0xFF] ^ (c >> 8);
        c ^= 0xFFFFFFFFu;                                                // crc32 of the piece (0 for an empty one)
        for (int k = 1; k < 64; k <<= 1) {
            const unsigned int o = __shfl_down(c, k, 64);
            if ((lane & (2 * k - 1)) == 0) {
                const long long ob = min((long long)len, (long long)(lane + k) * pl);
                const long long olen = min((long long)len, ob + (long long)k * pl) - ob;
                c = multmodp(x8nmodp(olen, x2n), c) ^ o;
            }
        }
        if (lane == 0) {
            unsigned int h = 0xFFFFFFFFu;
            const unsigned char type[4] = {'I', 'D', 'A', 'T'};
            for (int i = 0; i < 4; ++i) h = tab[(h ^ type[i]) & 0xFF] ^ (h >> 8);
            h ^= 0xFFFFFFFFu;
            if ((multmodp(x8nmodp(len, x2n), h) ^ c) != stored) atomicOr(&flags[f], kCorrupt);
        }
    }
}

// ------------------------------------------------------------------------------------------------ block finder
__global__ __launch_bounds__(kTabThreads) void finder_kernel(Geo g, const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                             unsigned long long* __restrict__ mask, long long* __restrict__ wcnt) {
    __shared__ Tabs tabs[kTabThreads];
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= g.NW) return;
    unsigned long long m = 0;
    if (!(g.flags & kNoFinder) && w * 8 < g.total_bytes) {
        int f = frame_of_byte(offsets, g.F, w * 8);
        for (int k = 0; k < 64; ++k) {
            const long long gb = w * 64 + k;
            if ((gb >> 3) >= g.total_bytes) break;
            while (f + 1 < g.F && offsets[f + 1] * 8 <= gb) ++f;
            const FrameView v = frame_view(data, offsets, f);
            long long pos = gb - offsets[f] * 8;
            if (pos < 16 || v.bs.n >= kMaxStream) continue;                // the zlib header
            if (((v.bs.peek(pos) >> 1) & 3u) != 2u) continue;
            pos += 3;
            if (dynamic_header(v.bs, pos, v.bits, tabs[threadIdx.x])) m |= 1ull << k;
        }
    }
    mask[w] = m;
    wcnt[w] = __popcll(m);
}

__global__ void compact_kernel(Geo g, const unsigned long long* __restrict__ mask, const long long* __restrict__ woff, long long* __restrict__ cand) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= g.NW) return;
    unsigned long long m = mask[w];
    long long i = woff[w];
    while (m && i < g.NCmax) {
        const int k = __ffsll((long long)m) - 1;
        cand[i++] = w * 64 + k;
        m &= m - 1;
    }
}

// ------------------------------------------------------------------------------------------------ speculative block decode
// One wave (a 64-thread workgroup) per candidate, grid-stride: lane 0 reads the header and builds the tables in LDS, then the wave
// decodes the body (wave_body, counting mode).
__global__ __launch_bounds__(64) void spec_kernel(Geo g, const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                  const long long* __restrict__ woff, const long long* __restrict__ cand,
                                                  long long* __restrict__ cend, long long* __restrict__ colen) {
    __shared__ Tabs tabs;
    __shared__ long long s_pos;
    __shared__ int s_ok;
    const long long nc = min(woff[g.NW], g.NCmax);
    for (long long i = blockIdx.x; i < nc; i += gridDim.x) {
        const long long gb = cand[i];
        const int f = frame_of_byte(offsets, g.F, gb >> 3);
        const FrameView v = frame_view(data, offsets, f);
        if (threadIdx.x == 0) {
            long long pos = gb - offsets[f] * 8 + 3;
            s_ok = dynamic_header(v.bs, pos, v.bits, tabs);
            s_pos = pos;
        }
        __syncthreads();
        long long end = -1, olen = 0;
        bool multi = false;
        if (s_ok && !wave_body(v.bs, s_pos, v.bits, tabs, 1 << ((v.bs.byte(0) >> 4) + 8), 0, g.raw, nullptr, g.sub_bits, &end, &olen, &multi))
            end = -1;
        if (threadIdx.x == 0) {
            cend[i] = end >= 0 ? end + offsets[f] * 8 : -1;
            colen[i] = olen;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ chain + serial backstop
__global__ __launch_bounds__(kTabThreads) void chain_kernel(Geo g, const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                            const long long* __restrict__ woff, const long long* __restrict__ cand,
                                                            const long long* __restrict__ cend, const long long* __restrict__ colen,
                                                            long long* __restrict__ bstart, long long* __restrict__ boff, int* __restrict__ flags,
                                                            long long* __restrict__ nblk) {
    __shared__ Tabs tabs[kTabThreads];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= g.F) return;
    nblk[f] = 0;
    if (flags[f] & kCorrupt) return;
    const FrameView v = frame_view(data, offsets, f);
    const long long nc = min(woff[g.NW], g.NCmax), base = slot_base(offsets, f), cap = v.bits / kMinBlockBits + 1;
    int fl = 0;
    bool ok = v.bs.n >= 6;
    if (ok) {
        const unsigned int cmf = v.bs.byte(0), flg = v.bs.byte(1);
        ok = (cmf & 15) == 8 && (cmf >> 4) <= 7 && ((cmf << 8) | flg) % 31 == 0 && !(flg & 0x20);
    }
    long long pos = 16, out = 0, n = 0;
    int fin = 0;
    while (ok && !fin) {
        if (n >= cap) { ok = false; break; }
        bstart[base + n] = pos;
        boff[base + n] = out;
        ++n;
        long long olen = -1, end = -1;
        if (((v.bs.peek(pos) >> 1) & 3u) == 2u) {
            const long long gb = pos + offsets[f] * 8;
            long long lo = 0, hi = nc;                                    // first candidate >= gb
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (cand[mid] < gb) lo = mid + 1; else hi = mid;
            }
            if (lo < nc && cand[lo] == gb && cend[lo] >= 0) {
                end = cend[lo] - offsets[f] * 8;
                olen = colen[lo];
                fin = (int)(v.bs.peek(pos) & 1u);
            }
        }
        if (end < 0) {
            fl |= kBackstop;
            ok = block(v.bs, pos, v.bits, tabs[threadIdx.x], out, g.raw, nullptr, &olen, &fin);
        } else {
            pos = end;
        }
        out += olen;
        if (out > g.raw) ok = false;
    }
    if (ok) {
        pos = (pos + 7) & ~7ll;                                            // the Adler-32 ends the stream exactly
        ok = pos / 8 + 4 == v.bs.n && out == g.raw;
    }
    flags[f] |= fl | (ok ? 0 : kCorrupt);
    nblk[f] = ok ? n : 0;
}

// ------------------------------------------------------------------------------------------------ write literals and sources
// One wave (a 64-thread workgroup) per confirmed block, grid-stride over the scan of the per-frame block counts: a stored block is
// copied by the lanes, a Huffman block decoded again by wave_body in writing mode from its exact start.
__global__ __launch_bounds__(64) void write_kernel(Geo g, const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                   const long long* __restrict__ bstart, const long long* __restrict__ boff,
                                                   const long long* __restrict__ bscan, int* __restrict__ flags, int* __restrict__ src) {
    __shared__ Tabs tabs;
    __shared__ long long s_pos;
    __shared__ int s_type, s_ok;
    const long long nb = bscan[g.F];
    for (long long i = blockIdx.x; i < nb; i += gridDim.x) {
        int lo = 0, hi = g.F - 1;                                       // the frame: the last f with bscan[f] <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (bscan[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const int f = lo;
        const long long slot = slot_base(offsets, f) + (i - bscan[f]);
        const FrameView v = frame_view(data, offsets, f);
        int* fsrc = src + (long long)f * g.raw;
        const long long o0 = boff[slot];
        if (threadIdx.x == 0) {
            long long pos = bstart[slot] + 1;
            const int type = (int)v.bs.get(pos, 2);
            int ok = 1;
            if (type == 1) fixed_tables(tabs);
            else if (type == 2) ok = dynamic_header(v.bs, pos, v.bits, tabs);
            else if (type == 0) pos = ((pos + 7) & ~7ll) + 32;           // the stored bytes (their length was checked by the chain)
            else ok = 0;
            s_type = type;
            s_ok = ok;
            s_pos = pos;
        }
        __syncthreads();
        bool ok = s_ok;
        bool multi = false;
        if (ok && s_type == 0) {
            const long long ln = v.bs.peek(s_pos - 32) & 0xFFFFu;
            for (long long k = threadIdx.x; k < ln; k += 64)
                if (o0 + k < g.raw) fsrc[o0 + k] = -1 - (int)v.bs.byte((s_pos >> 3) + k);
        } else if (ok) {
            long long end, olen;
            ok = wave_body(v.bs, s_pos, v.bits, tabs, 1 << ((v.bs.byte(0) >> 4) + 8), o0, g.raw, fsrc, g.sub_bits, &end, &olen, &multi);
        }
        if (threadIdx.x == 0 && (!ok || multi)) atomicOr(&flags[f], (ok ? 0 : kCorrupt) | (multi ? kMultiRound : 0));
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ resolve, check, unfilter, colour
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

__global__ __launch_bounds__(kFrameThreads) void frame_kernel(Geo g, const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                              int* __restrict__ flags, int* __restrict__ src_all, unsigned char* __restrict__ px_all,
                                                              unsigned char* __restrict__ out, unsigned char* __restrict__ status) {
    __shared__ int s_flags, s_more;
    __shared__ unsigned long long s_a[kFrameThreads], s_b[kFrameThreads];
    const int f = blockIdx.x, t = threadIdx.x;
    if (t == 0) s_flags = flags[f];
    __syncthreads();
    if (s_flags & kCorrupt) {
        if (t == 0) status[f] = (unsigned char)(s_flags & (kCorrupt | kMultiRound | kBackstop));
        return;
    }
    const long long n = g.raw;
    int* src = src_all + (long long)f * n;
    unsigned char* px = px_all + (long long)f * n;
    // pointer jumping: every source index is an earlier byte, so the chains end at literals
    for (;;) {
        if (t == 0) s_more = 0;
        __syncthreads();
        int more = 0;
        for (long long i = t; i < n; i += kFrameThreads) {
            const int s = src[i];
            if (s >= 0) {
                const int s2 = src[s];
                src[i] = s2;
                more |= s2 >= 0;
            }
        }
        if (more) s_more = 1;
        __syncthreads();
        const int again = s_more;
        __syncthreads();
        if (!again) break;
    }
    // gather and Adler-32: a = 1 + sum d_i, b = n + sum (n - i) d_i, mod 65521
    unsigned long long sa = 0, sb = 0;
    for (long long i = t; i < n; i += kFrameThreads) {
        const unsigned int d = (unsigned int)(-1 - src[i]) & 0xFFu;
        px[i] = (unsigned char)d;
        sa += d;
        sb += (unsigned long long)(n - i) * d;
    }
    s_a[t] = sa % 65521u;
    s_b[t] = sb % 65521u;
    __syncthreads();
    for (int k = kFrameThreads / 2; k > 0; k >>= 1) {
        if (t < k) {
            s_a[t] = (s_a[t] + s_a[t + k]) % 65521u;
            s_b[t] = (s_b[t] + s_b[t + k]) % 65521u;
        }
        __syncthreads();
    }
    const long long S = 1 + (long long)g.W * g.C;
    if (t == 0) {
        const unsigned int a = (unsigned int)((1 + s_a[0]) % 65521u), b = (unsigned int)(((unsigned long long)n % 65521u + s_b[0]) % 65521u);
        const unsigned char* e = data + offsets[f + 1] - 4;
        const unsigned int stored = ((unsigned int)e[0] << 24) | ((unsigned int)e[1] << 16) | ((unsigned int)e[2] << 8) | e[3];
        if (((b << 16) | a) != stored) s_flags |= kCorrupt;
    }
    __syncthreads();
    for (int r = t; r < g.H; r += kFrameThreads)
        if (px[r * S] > 4) atomicOr(&s_flags, kCorrupt);
    __syncthreads();
    if (s_flags & kCorrupt) {
        if (t == 0) {
            flags[f] = s_flags;
            status[f] = (unsigned char)(s_flags & (kCorrupt | kMultiRound | kBackstop));
        }
        return;
    }
    // unfilter as a diagonal wavefront: row r handles pixel x = step - (r - r0), one pixel behind the row above
    const int C = g.C;
    unsigned char* o = out + (long long)f * g.H * g.W * 3;
    for (int r0 = 0; r0 < g.H; r0 += kFrameThreads) {
        const int rows = min(kFrameThreads, g.H - r0), r = r0 + t;
        unsigned char* cur = px + (long long)r * S + 1;
        const unsigned char* up = cur - S;
        const int ft = t < rows ? px[(long long)r * S] : 0;
        for (int step = 0; step < g.W + rows - 1; ++step) {
            const int x = step - t;
            if (t < rows && x >= 0 && x < g.W) {
                unsigned char v[4];
                for (int c = 0; c < C; ++c) {
                    const int j = x * C + c;
                    const int a = x > 0 ? cur[j - C] : 0, b = r > 0 ? up[j] : 0, cc = (x > 0 && r > 0) ? up[j - C] : 0;
                    int p = cur[j];
                    if (ft == 1) p += a;
                    else if (ft == 2) p += b;
                    else if (ft == 3) p += (a + b) >> 1;
                    else if (ft == 4) p += paeth(a, b, cc);
                    cur[j] = v[c] = (unsigned char)p;
                }
                unsigned char* q = o + ((long long)r * g.W + x) * 3;
                if (C <= 2) {
                    q[0] = q[1] = q[2] = v[0];
                } else {
                    q[0] = v[2];
                    q[1] = v[1];
                    q[2] = v[0];
                }
            }
            __syncthreads();
        }
    }
    if (t == 0) status[f] = (unsigned char)(s_flags & (kCorrupt | kMultiRound | kBackstop));
}

int check_args(int F, int H, int W, int C, long long total_bytes, int sub_bits, int flags, Geo& g, const char* who) {
    SS_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "%s: bad dims F=%d H=%d W=%d", who, F, H, W);
    SS_CHECK_ARG(C == 1 || C == 2 || C == 3 || C == 4, "%s: channels=%d (1, 2, 3 or 4)", who, C);
    SS_CHECK_ARG(total_bytes >= 0 && total_bytes < (1ll << 32), "%s: total_bytes=%lld", who, (long long)total_bytes);
    SS_CHECK_ARG(sub_bits == 0 || (sub_bits >= 64 && sub_bits % 64 == 0 && sub_bits <= 65536), "%s: sub_bits=%d (0, or a multiple of 64 in [64, 65536])",
                 who, sub_bits);
    SS_CHECK_ARG(flags == 0 || flags == kNoFinder, "%s: flags=%d (0 or 1)", who, flags);
    const long long raw = (long long)H * (1 + (long long)W * C);
    SS_CHECK_ARG(raw < (1ll << 31) && (long long)F * raw < (1ll << 40), "%s: %d frames of %d x %d x %d are too large for one call", who, F, H, W, C);
    g.F = F;
    g.H = H;
    g.W = W;
    g.C = C;
    g.flags = flags;
    g.sub_bits = sub_bits ? sub_bits : kDefaultSubBits;
    g.raw = raw;
    g.total_bytes = total_bytes;
    g.NW = cdiv(total_bytes, 8) + 1;
    g.NCmax = total_bytes / 8 + 64;
    g.NB = total_bytes * 8 / kMinBlockBits + F + 1;
    g.NCH = total_bytes + F;
    return STEMSEG_OK;
}

}  // namespace

extern "C" size_t stemseg_hip_png_decode_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t channels, int64_t total_bytes, int32_t sub_bits,
                                                        int32_t flags) {
    Geo g;
    if (check_args(F, H, W, channels, total_bytes, sub_bits, flags, g, "png_decode_workspace_bytes") != STEMSEG_OK) return 0;
    return layout(nullptr, g).bytes;
}

extern "C" int stemseg_hip_png_decode(const uint8_t* data, const int64_t* offsets, const void* headers, int32_t F, int32_t H, int32_t W,
                                      int32_t channels, int64_t total_bytes, int32_t sub_bits, int32_t flags, void* workspace, size_t ws_bytes,
                                      uint8_t* out, uint8_t* status, void* stream) {
    Geo g;
    int rc = check_args(F, H, W, channels, total_bytes, sub_bits, flags, g, "png_decode");
    if (rc != STEMSEG_OK) return rc;
    SS_CHECK_ARG(data && offsets && headers && workspace && out && status, "png_decode: null pointer");
    Ws w = layout(static_cast<char*>(workspace), g);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "png_decode: workspace %zu bytes < %zu", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const long long* off = reinterpret_cast<const long long*>(offsets);
    const long long* hdr = static_cast<const long long*>(headers);
    const unsigned int* recs = reinterpret_cast<const unsigned int*>(hdr + (long long)F * kHdrWords);
    hipLaunchKernelGGL(init_kernel, dim3(grid(F)), dim3(kThreads), 0, s, g, off, hdr, w.flags);
    hipLaunchKernelGGL(crc_kernel, dim3((int)std::min<long long>(cdiv(g.NCH, kThreads / 64), 2048)), dim3(kThreads), 0, s, g, data, off, hdr, recs,
                       w.flags);
    hipLaunchKernelGGL(finder_kernel, dim3(grid(g.NW, kTabThreads)), dim3(kTabThreads), 0, s, g, data, off, w.mask, w.wcnt);
    launch_scan(w.wcnt, nullptr, g.NW, w.tile_sums, w.woff, s);
    hipLaunchKernelGGL(compact_kernel, dim3(grid(g.NW)), dim3(kThreads), 0, s, g, w.mask, w.woff, w.cand);
    hipLaunchKernelGGL(spec_kernel, dim3((int)std::min<long long>(g.NCmax, kWaveGrid)), dim3(64), 0, s, g, data, off, w.woff, w.cand, w.cend, w.colen);
    hipLaunchKernelGGL(chain_kernel, dim3(grid(F, kTabThreads)), dim3(kTabThreads), 0, s, g, data, off, w.woff, w.cand, w.cend, w.colen, w.bstart,
                       w.boff, w.flags, w.nblk);
    launch_scan(w.nblk, nullptr, F, w.tile_sums, w.bscan, s);
    hipLaunchKernelGGL(write_kernel, dim3((int)std::min<long long>(g.NB, kWaveGrid)), dim3(64), 0, s, g, data, off, w.bstart, w.boff, w.bscan, w.flags, w.src);
    hipLaunchKernelGGL(frame_kernel, dim3(F), dim3(kFrameThreads), 0, s, g, data, off, w.flags, w.src, w.px, out, status);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
