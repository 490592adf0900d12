// Baseline JPEG decoder, pixel-identical to libjpeg-turbo's default decompression (islow IDCT, fancy upsampling, table-driven
// YCbCr -> RGB) as PIL and cv2.imread drive it.  F frames of one geometry (size, sampling, components) per call; each frame has its
// own tables (a blob per frame, stemseg_amd/utils/jpeg.py) and its own restart interval.  Stages, a fixed launch count whatever the data:
//   unstuff  : one thread per 256-byte chunk of a frame's entropy-coded segment counts its kept bytes and RSTn markers (0xFF00 ->
//              0xFF; an 0xFF followed by anything else is corruption); the exact scan (scan.h) gives every kept byte its place.
//              Each restart interval is written at a subsequence-aligned offset of the frame's bit stream, so a subsequence never
//              straddles two intervals and the first subsequence of an interval starts from a known decoder state
//   huffman  : the self-synchronising scheme of Weissenberger & Schmidt (ICPP 2018).  The stream is cut into subsequences of
//              sub_bits bits.  spec: each decodes speculatively from (its first bit, block 0 of the MCU, DC) until it passes
//              its end; the exit state is (bit position, block within the MCU, zigzag index).  sync (two launches, buffers
//              swapped): inside a workgroup of 256 subsequences, each re-decodes from its predecessor's exit state, with
//              barriers between rounds, until no exit state changes (at most max_rounds rounds); across workgroups the
//              predecessor state is the previous launch's.  converge: a frame has converged when every subsequence's input is
//              its predecessor's final exit.  serial: one thread per restart interval of an unconverged frame walks its
//              subsequences in order (the exact backstop; returns at once for converged frames)
//   blocks   : the per-subsequence block counts are scanned; every interval must hold exactly its MCUs' blocks.  write: each
//              subsequence decodes again from its exact state and writes the blocks it starts (DC difference, AC in natural order)
//   dc       : segmented scan per (frame, component) in coding order, reset at every restart (int32 wrap, stored as int16)
//   idct     : one thread per block: dequantise (int16 multiplier table) and islow IDCT (jidctint.c) with the range-limit table
//              and its RANGE_MASK wrap, into component planes of whole MCUs
//   color    : 4 pixels per thread: fancy upsampling (jdsample.c h2v1 / h2v2, context rows replicated at the top and bottom,
//              plain replication when the chroma is at most 2 samples wide) and jdcolor.c's tables; BGR with 4-byte stores
// Status per frame: bit 0 corrupt (invalid code, k > 63, a segment exhausted inside a block, a wrong RST sequence, an interval
// with the wrong number of blocks, a stray marker): the frame's pixels are undefined and the caller decodes it on the host;
// bit 1 the synchronisation took more than one round; bit 2 the serial backstop decoded it.
#include "common.h"
#include "scan.h"

#include <algorithm>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 256;                   // bytes per unstuffing chunk
constexpr int kHdr = 64, kQuant = 512, kHuff = 912;
constexpr int kBlobBytes = kHdr + kQuant + 8 * kHuff;
constexpr int kDefaultSubBits = 512;
constexpr int kDefaultRounds = 256;           // a whole workgroup: a local chain always converges
constexpr int kSyncLaunches = 2;
constexpr long long kMaxEcs = 1ll << 27;      // frame-local bit positions stay in int32

enum : int { kCorrupt = 1, kMultiRound = 2, kBackstop = 4, kUnconverged = 8 };

__host__ __device__ __forceinline__ long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
__host__ __device__ __forceinline__ long long rup(long long a, long long b) { return cdiv(a, b) * b; }
__host__ __device__ __forceinline__ long long lmax(long long a, long long b) { return a > b ? a : b; }

__constant__ unsigned char kNat[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                                       7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                       39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct FrameDesc {
    long long begin, len;                     // entropy-coded segment in `data`
    int chunk_base, n_chunks, int_base, n_int, ri, sub_base, sub_cap, pad;
};

struct Geo {
    int F, H, W, nc, hs, vs;                  // luma sampling (1 for grayscale)
    int mw, mh, n_mcu, bpm, nblk;             // MCUs, blocks per MCU, blocks per frame
    int pw[3], ph[3];                         // component plane sizes (whole MCUs)
    long long poff[3], pframe;                // plane offsets within a frame's planes, bytes per frame
    int sub_bits, rounds;
    long long NC, NI, NS;                     // caps: chunks, intervals, subsequences (a multiple of 256)
};

bool make_geo(int F, int H, int W, int sampling, long long total_bytes, long long total_intervals, int sub_bits, int rounds, Geo& g) {
    g.F = F;
    g.H = H;
    g.W = W;
    if (sampling == 0) {
        g.nc = 1;
        g.hs = g.vs = 1;
    } else {
        g.nc = 3;
        g.hs = sampling >> 4;
        g.vs = sampling & 15;
        if (!((g.hs == 1 && g.vs == 1) || (g.hs == 2 && g.vs == 1) || (g.hs == 2 && g.vs == 2)) || (sampling >> 8)) return false;
    }
    g.mw = (int)cdiv(W, 8 * g.hs);
    g.mh = (int)cdiv(H, 8 * g.vs);
    g.n_mcu = g.mw * g.mh;
    g.bpm = g.hs * g.vs + (g.nc - 1);
    g.nblk = g.n_mcu * g.bpm;
    long long o = 0;
    for (int c = 0; c < 3; ++c) {
        const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
        g.pw[c] = g.mw * h * 8;
        g.ph[c] = g.mh * v * 8;
        g.poff[c] = o;
        if (c < g.nc) o += (long long)g.pw[c] * g.ph[c];
    }
    g.pframe = rup(o, 16);
    g.sub_bits = sub_bits ? sub_bits : kDefaultSubBits;
    g.rounds = rounds ? rounds : kDefaultRounds;
    g.NC = total_bytes / kChunk + F;
    g.NI = total_intervals;
    g.NS = rup(cdiv(total_bytes * 8, g.sub_bits) + (long long)F * kThreads + total_intervals, kThreads);
    return true;
}

struct Ws {
    FrameDesc* desc;
    int* flags;
    long long* ccnt;          // [NC] kept bytes | RST markers << 32
    long long* coff;          // [NC + 1]
    int* istart;              // [NI] unstuffed byte where interval k starts (frame-local)
    int* ilen;                // [NI]
    long long* isubs;         // [NI] subsequences of interval k (>= 1)
    long long* isoff;         // [NI + 1]
    unsigned char* stream;    // [NS * sub_bits / 8]
    int* skind;               // [NS] frame-local interval of the subsequence, -1 beyond the frame's data
    int* send;                // [NS] end bit of that interval's data (frame-local)
    unsigned long long* st[2];// [NS] exit states, double-buffered across sync launches
    unsigned long long* sin;  // [NS] the input state of the last decode
    long long* cnt;           // [NS] blocks started
    long long* boff;          // [NS + 1]
    int* dcdiff;              // [F * nblk]
    short* coef;              // [F * nblk][64] natural order
    unsigned char* planes;    // [F][pframe]
    long long* tile_sums;
    size_t bytes;
};

Ws layout(char* base, const Geo& g) {
    Ws w{};
    size_t o = 0;
    auto take = [&](long long n) { void* p = base ? base + o : nullptr; o += rup(lmax(n, 1), 256); return p; };
    const long long NB = (long long)g.F * g.nblk;
    w.desc = (FrameDesc*)take(sizeof(FrameDesc) * g.F);
    w.flags = (int*)take(4 * g.F);
    w.ccnt = (long long*)take(8 * g.NC);
    w.coff = (long long*)take(8 * (g.NC + 1));
    w.istart = (int*)take(4 * g.NI);
    w.ilen = (int*)take(4 * g.NI);
    w.isubs = (long long*)take(8 * g.NI);
    w.isoff = (long long*)take(8 * (g.NI + 1));
    w.stream = (unsigned char*)take(g.NS * (g.sub_bits / 8) + 8);
    w.skind = (int*)take(4 * g.NS);
    w.send = (int*)take(4 * g.NS);
    w.st[0] = (unsigned long long*)take(8 * g.NS);
    w.st[1] = (unsigned long long*)take(8 * g.NS);
    w.sin = (unsigned long long*)take(8 * g.NS);
    w.cnt = (long long*)take(8 * g.NS);
    w.boff = (long long*)take(8 * (g.NS + 1));
    w.dcdiff = (int*)take(4 * NB);
    w.coef = (short*)take(128 * NB);
    w.planes = (unsigned char*)take(g.pframe * g.F);
    w.tile_sums = (long long*)take(8 * (scan_tiles(std::max(std::max(g.NC, g.NI), g.NS)) + 1));
    w.bytes = o;
    return w;
}

int grid(long long n) { return (int)std::max<long long>(1, cdiv(n, kThreads)); }

// the frame whose range of chunks (kField 0) / intervals (1) / subsequences (2) holds i, or -1
template <int kField>
__device__ __forceinline__ int frame_of(const FrameDesc* d, int F, long long i) {
    auto base = [&](int f) { return kField == 0 ? d[f].chunk_base : kField == 1 ? d[f].int_base : d[f].sub_base; };
    auto size = [&](int f) { return kField == 0 ? d[f].n_chunks : kField == 1 ? d[f].n_int : d[f].sub_cap; };
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base(mid) <= i) lo = mid;
        else hi = mid - 1;
    }
    return (i >= base(lo) && i < (long long)base(lo) + size(lo)) ? lo : -1;
}

// ------------------------------------------------------------------------------------------------ setup and unstuffing
__global__ void setup_kernel(const long long* __restrict__ ecs, const unsigned char* __restrict__ tables, Geo g, FrameDesc* __restrict__ desc,
                             int* __restrict__ flags) {
    if (threadIdx.x != 0) return;
    long long cb = 0, ib = 0, sb = 0;
    for (int f = 0; f < g.F; ++f) {
        FrameDesc d{};
        d.begin = ecs[2 * f];
        d.len = ecs[2 * f + 1] - ecs[2 * f];
        const int ri = reinterpret_cast<const int*>(tables + (long long)f * kBlobBytes)[0];
        d.ri = ri > 0 ? min(ri, g.n_mcu) : g.n_mcu;
        d.n_int = (int)cdiv(g.n_mcu, d.ri);
        const long long len = lmax(d.len, 0);
        const long long nch = cdiv(len, kChunk), cap = rup(cdiv(len * 8, g.sub_bits) + d.n_int, kThreads);
        int fl = 0;
        if (d.len < 0 || d.len >= kMaxEcs || cb + nch > g.NC || ib + d.n_int > g.NI || sb + cap > g.NS) {
            fl = kCorrupt;                    // inconsistent with the caps the caller sized the workspace for: left to the host
            d.len = 0;
            d.n_int = 0;
        }
        d.chunk_base = (int)cb;
        d.n_chunks = fl ? 0 : (int)nch;
        d.int_base = (int)ib;
        d.sub_base = (int)sb;
        d.sub_cap = fl ? 0 : (int)cap;
        cb += d.n_chunks;
        ib += d.n_int;
        sb += d.sub_cap;
        desc[f] = d;
        flags[f] = fl;
    }
}

__global__ void interval_init_kernel(Geo g, int* __restrict__ istart) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < g.NI) istart[k] = 0;
}

// byte i of a segment [b, e): 0 kept, 1 dropped, 2 dropped RST marker (the byte after its 0xFF), -1 corrupt
__device__ __forceinline__ int byte_class(const unsigned char* d, long long b, long long e, long long i) {
    const int cur = d[i];
    if (i > b && d[i - 1] == 0xFF) {
        if (cur == 0) return 1;
        if (cur >= 0xD0 && cur <= 0xD7) return 2;
        return -1;
    }
    if (cur == 0xFF) {
        if (i + 1 >= e) return -1;
        const int nx = d[i + 1];
        if (nx == 0) return 0;
        if (nx >= 0xD0 && nx <= 0xD7) return 1;
        return -1;
    }
    return 0;
}

__global__ __launch_bounds__(kThreads) void chunk_count_kernel(const unsigned char* __restrict__ data, Geo g, const FrameDesc* __restrict__ desc,
                                                              int* __restrict__ flags, long long* __restrict__ ccnt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.NC) return;
    const int f = frame_of<0>(desc, g.F, i);
    long long v = 0;
    if (f >= 0) {
        const FrameDesc d = desc[f];
        const long long b = d.begin, e = d.begin + d.len, s = b + (i - d.chunk_base) * kChunk;
        long long kept = 0, rst = 0;
        bool bad = false;
        for (long long k = s; k < min(e, s + kChunk); ++k) {
            const int c = byte_class(data, b, e, k);
            kept += c == 0;
            rst += c == 2;
            bad |= c < 0;
        }
        if (bad) atomicOr(flags + f, kCorrupt);
        v = kept | (rst << 32);
    }
    ccnt[i] = v;
}

__global__ __launch_bounds__(kThreads) void rst_kernel(const unsigned char* __restrict__ data, Geo g, const FrameDesc* __restrict__ desc,
                                                      const long long* __restrict__ coff, int* __restrict__ flags, int* __restrict__ istart) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.NC) return;
    const int f = frame_of<0>(desc, g.F, i);
    if (f < 0) return;
    const FrameDesc d = desc[f];
    const long long b = d.begin, e = d.begin + d.len, s = b + (i - d.chunk_base) * kChunk;
    const long long c0 = coff[d.chunk_base];
    long long kept = (coff[i] & 0xFFFFFFFFll) - (c0 & 0xFFFFFFFFll), r = (coff[i] >> 32) - (c0 >> 32);
    for (long long k = s; k < min(e, s + kChunk); ++k) {
        const int c = byte_class(data, b, e, k);
        if (c == 0) ++kept;
        if (c == 2) {
            if ((int)data[k] - 0xD0 != (int)(r & 7) || r + 1 >= d.n_int) atomicOr(flags + f, kCorrupt);
            else istart[d.int_base + r + 1] = (int)kept;
            ++r;
        }
    }
}

__global__ void interval_len_kernel(Geo g, const FrameDesc* __restrict__ desc, const long long* __restrict__ coff, const int* __restrict__ istart,
                                    int* __restrict__ flags, int* __restrict__ ilen, long long* __restrict__ isubs) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= g.NI) return;
    const int f = frame_of<1>(desc, g.F, k);
    if (f < 0) {
        ilen[k] = 0;
        isubs[k] = 0;
        return;
    }
    const FrameDesc d = desc[f];
    const long long lo = coff[d.chunk_base], hi = coff[d.chunk_base + d.n_chunks];
    const long long total = (hi & 0xFFFFFFFFll) - (lo & 0xFFFFFFFFll), n_rst = (hi >> 32) - (lo >> 32);
    const int kk = (int)(k - d.int_base);
    if (kk == 0 && n_rst != d.n_int - 1) atomicOr(flags + f, kCorrupt);
    const long long s = istart[k], e = kk + 1 < d.n_int ? istart[k + 1] : total;
    const long long len = lmax(0, e - s);
    ilen[k] = (int)len;
    isubs[k] = lmax(1, cdiv(len * 8, g.sub_bits));
}

__global__ __launch_bounds__(kThreads) void scatter_kernel(const unsigned char* __restrict__ data, Geo g, const FrameDesc* __restrict__ desc,
                                                          const long long* __restrict__ coff, const int* __restrict__ istart,
                                                          const int* __restrict__ ilen, const long long* __restrict__ isoff,
                                                          unsigned char* __restrict__ stream) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.NC) return;
    const int f = frame_of<0>(desc, g.F, i);
    if (f < 0) return;
    const FrameDesc d = desc[f];
    const long long b = d.begin, e = d.begin + d.len, s = b + (i - d.chunk_base) * kChunk;
    const long long c0 = coff[d.chunk_base];
    long long u = (coff[i] & 0xFFFFFFFFll) - (c0 & 0xFFFFFFFFll), r = (coff[i] >> 32) - (c0 >> 32);
    const int sb = g.sub_bits / 8;
    unsigned char* out = stream + (long long)d.sub_base * sb;
    const long long cap = (long long)d.sub_cap * sb;
    for (long long k = s; k < min(e, s + kChunk); ++k) {
        const int c = byte_class(data, b, e, k);
        if (c == 2) ++r;
        if (c != 0) continue;
        if (r < d.n_int) {
            const long long q = u - istart[d.int_base + r];
            const long long o = (isoff[d.int_base + r] - isoff[d.int_base]) * sb + q;
            if (q >= 0 && q < ilen[d.int_base + r] && o >= 0 && o < cap) out[o] = data[k];
        }
        ++u;
    }
}

__global__ __launch_bounds__(kThreads) void sub_info_kernel(Geo g, const FrameDesc* __restrict__ desc, const int* __restrict__ ilen,
                                                           const long long* __restrict__ isoff, int* __restrict__ flags, int* __restrict__ skind,
                                                           int* __restrict__ send) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.NS) return;
    const int f = frame_of<2>(desc, g.F, j);
    skind[j] = -1;
    send[j] = 0;
    if (f < 0) return;
    const FrameDesc d = desc[f];
    const long long* o = isoff + d.int_base;
    const long long jl = j - d.sub_base, used = o[d.n_int] - o[0];
    if (jl == 0 && used > d.sub_cap) atomicOr(flags + f, kCorrupt);
    if (d.n_int == 0 || jl >= used || jl >= d.sub_cap) return;
    int lo = 0, hi = d.n_int - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (o[mid] - o[0] <= jl) lo = mid;
        else hi = mid - 1;
    }
    skind[j] = lo;
    send[j] = (int)((o[lo] - o[0]) * g.sub_bits + 8ll * ilen[d.int_base + lo]);
}

// ------------------------------------------------------------------------------------------------ Huffman decoding
// decoder state: (bit position << 16) | (block within the MCU << 8) | zigzag index (0 = the next symbol is a DC)
__device__ __forceinline__ unsigned long long pack(int p, int c, int z) { return ((unsigned long long)(unsigned)p << 16) | ((unsigned)c << 8) | (unsigned)z; }
__device__ __forceinline__ int st_p(unsigned long long s) { return (int)(s >> 16); }
__device__ __forceinline__ int st_c(unsigned long long s) { return (int)((s >> 8) & 255); }
__device__ __forceinline__ int st_z(unsigned long long s) { return (int)(s & 255); }

struct Frame {
    const unsigned char* s;                   // the frame's bit stream
    const unsigned char* blob;
    int bpm, comp_of[6];
};

// 32 bits from bit p, zeros from bit `end` on (end is a multiple of 8); never reads a byte at or past end
__device__ __forceinline__ unsigned int peek32(const unsigned char* s, int p, int end) {
    const int b0 = p >> 3, e = end >> 3;
    unsigned long long v = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) v = (v << 8) | (b0 + k < e ? s[b0 + k] : 0u);
    return (unsigned int)(v >> (8 - (p & 7)));
}

// symbol of the table at `t` for the bits left-aligned in `bits`, its code length in len; -1 for an invalid code
__device__ __forceinline__ int huff(const unsigned char* t, unsigned int bits, int& len) {
    const unsigned int look = reinterpret_cast<const unsigned short*>(t)[bits >> 24];
    if (look) {
        len = (int)(look >> 8);
        return (int)(look & 255);
    }
    const int* maxcode = reinterpret_cast<const int*>(t + 512);
    const int* valoff = reinterpret_cast<const int*>(t + 584);
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(bits >> (32 - l));
        if (code <= maxcode[l]) {
            len = l;
            return t[656 + ((code + valoff[l]) & 255)];
        }
    }
    return -1;
}

__device__ __forceinline__ int extend(unsigned int v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

__device__ __forceinline__ const unsigned char* dc_tab(const Frame& fr, int comp) {
    return fr.blob + kHdr + kQuant + (reinterpret_cast<const int*>(fr.blob)[2 + comp] & 3) * kHuff;
}
__device__ __forceinline__ const unsigned char* ac_tab(const Frame& fr, int comp) {
    return fr.blob + kHdr + kQuant + (4 + (reinterpret_cast<const int*>(fr.blob)[5 + comp] & 3)) * kHuff;
}

// An invalid code, a DC category above 15 or k > 63.  Writing (from an exact state) it is corruption.  Decoding speculatively it
// only means a wrong start state: step one bit and expect a DC, so that the decode keeps moving and can fall into step with the
// true one -- a stuck state would be handed down the whole chain and never synchronise.
#define BAD_SYMBOL()          \
    if (kWrite) {             \
        err = 1;              \
        break;                \
    }                         \
    p += 1;                   \
    z = 0;                    \
    continue

// Decodes from state (p, c, z) in the interval whose data ends at bit `iend`.  kWrite = false: stops at the first symbol boundary
// at or past `stop`; kWrite = true: stops at the first block boundary at or past `stop` and writes every block it starts (block
// index blk0, blk0 + 1, ... < nblk).  Stops early -- state unchanged -- at the end of the interval (padding of fewer than 8 one
// bits, or a symbol that would run past iend); when writing, also on an invalid code / k > 63 (err = 1, as is running out
// inside a block).  Returns the blocks started.
template <bool kWrite>
__device__ int decode_run(const Frame& fr, int& p, int& c, int& z, int stop, int iend, int& err, long long blk0 = 0, int nblk = 0,
                          int* dcdiff = nullptr, short* coef = nullptr) {
    int started = 0;
    const unsigned char* tab = z ? ac_tab(fr, fr.comp_of[c]) : nullptr;
    short* blk = nullptr;
    while (kWrite ? (z != 0 || p < stop) : p < stop) {
        const unsigned int bits = peek32(fr.s, p, iend);
        int len = 0;
        if (z == 0) {
            const int rem = iend - p;
            if (rem < 8 && (rem <= 0 || (bits >> (32 - rem)) == (1u << rem) - 1u)) break;
            const int s = huff(dc_tab(fr, fr.comp_of[c]), bits, len);
            if (s < 0 || s > 15) {
                BAD_SYMBOL();
            }
            if (p + len + s > iend) break;
            if (kWrite) {
                const long long b = blk0 + started;
                if (b >= nblk) {
                    err = 1;
                    break;
                }
                dcdiff[b] = s ? extend(peek32(fr.s, p + len, iend) >> (32 - s), s) : 0;
                blk = coef + 64 * b;
            }
            ++started;
            p += len + s;
            z = 1;
            tab = ac_tab(fr, fr.comp_of[c]);
            continue;
        }
        const int rs = huff(tab, bits, len);
        if (rs < 0) {
            BAD_SYMBOL();
        }
        const int r = rs >> 4, s = rs & 15;
        if (p + len + s > iend) {
            if (kWrite) err = 1;
            break;
        }
        int nz = z;
        if (s) {
            nz += r;
            if (nz > 63) {
                BAD_SYMBOL();
            }
            if (kWrite && blk) blk[kNat[nz]] = (short)extend(peek32(fr.s, p + len, iend) >> (32 - s), s);
            ++nz;
        } else if (r == 15) {
            nz += 16;
            if (nz > 64) {
                BAD_SYMBOL();
            }
        } else {
            nz = 64;
        }
        p += len + s;
        z = nz;
        if (z >= 64) {
            z = 0;
            c = c + 1 == fr.bpm ? 0 : c + 1;
            blk = nullptr;
        }
    }
    return started;
}

__device__ __forceinline__ Frame frame_view(const Geo& g, const FrameDesc& d, int f, const unsigned char* stream, const unsigned char* tables) {
    Frame fr;
    fr.s = stream + (long long)d.sub_base * (g.sub_bits / 8);
    fr.blob = tables + (long long)f * kBlobBytes;
    fr.bpm = g.bpm;
    int k = 0;
    for (int i = 0; i < g.hs * g.vs; ++i) fr.comp_of[k++] = 0;
    for (int c = 1; c < g.nc; ++c) fr.comp_of[k++] = c;
    for (; k < 6; ++k) fr.comp_of[k] = 0;
    return fr;
}

// subsequence j is the first of its restart interval (its input state is known: its first bit, block 0, DC)
__device__ __forceinline__ bool is_first(const FrameDesc& d, const long long* isoff, const int* skind, long long j) {
    const int k = skind[j];
    return k >= 0 && j - d.sub_base == isoff[d.int_base + k] - isoff[d.int_base];
}

__global__ __launch_bounds__(kThreads) void spec_kernel(Geo g, const FrameDesc* __restrict__ desc, const unsigned char* __restrict__ tables,
                                                       const unsigned char* __restrict__ stream, const int* __restrict__ skind,
                                                       const int* __restrict__ send, unsigned long long* __restrict__ st,
                                                       unsigned long long* __restrict__ sin, long long* __restrict__ cnt) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.NS) return;
    const int f = frame_of<2>(desc, g.F, j);
    int p = 0, c = 0, z = 0, n = 0;
    if (f >= 0) {
        const FrameDesc d = desc[f];
        p = (int)(j - d.sub_base) * g.sub_bits;
        sin[j] = pack(p, 0, 0);
        if (skind[j] >= 0) {
            const Frame fr = frame_view(g, d, f, stream, tables);
            int err = 0;
            n = decode_run<false>(fr, p, c, z, p + g.sub_bits, send[j], err);
        }
    } else {
        sin[j] = 0;
    }
    st[j] = pack(p, c, z);
    cnt[j] = n;
}

__global__ __launch_bounds__(kThreads) void sync_kernel(Geo g, int launch, const FrameDesc* __restrict__ desc, const unsigned char* __restrict__ tables,
                                                       const unsigned char* __restrict__ stream, const int* __restrict__ skind,
                                                       const int* __restrict__ send, const long long* __restrict__ isoff,
                                                       const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst,
                                                       unsigned long long* __restrict__ sin, long long* __restrict__ cnt, int* __restrict__ flags) {
    __shared__ unsigned long long lds[kThreads];
    const int t = threadIdx.x;
    const long long j = (long long)blockIdx.x * blockDim.x + t;     // NS is a multiple of 256: every thread has a j
    const int f = frame_of<2>(desc, g.F, j);                        // one frame per workgroup (sub_base, sub_cap: multiples of 256)
    const bool live = f >= 0 && skind[j] >= 0;
    FrameDesc d{};
    Frame fr{};
    bool first = false;
    unsigned long long cur = src[j], prev_in = sin[j], in = 0;
    if (live) {
        d = desc[f];
        fr = frame_view(g, d, f, stream, tables);
        first = is_first(d, isoff, skind, j);
        in = first ? prev_in : (t == 0 ? src[j - 1] : 0ull);
    }
    long long n = cnt[j];
    int changed_rounds = 0;
    lds[t] = cur;
    __syncthreads();
    for (int r = 0; r < g.rounds; ++r) {
        if (live && !first && t > 0) in = lds[t - 1];
        int changed = 0;
        if (live && in != prev_in) {
            int p = st_p(in), c = st_c(in), z = st_z(in), err = 0;
            n = decode_run<false>(fr, p, c, z, (int)(j - d.sub_base + 1) * g.sub_bits, send[j], err);
            const unsigned long long o = pack(p, c, z);
            changed = o != cur;
            cur = o;
            prev_in = in;
        }
        __syncthreads();
        lds[t] = cur;
        if (!__syncthreads_or(changed)) break;
        ++changed_rounds;
    }
    dst[j] = cur;
    if (live) {
        sin[j] = prev_in;
        cnt[j] = n;
        if (t == 0 && changed_rounds > (launch == 0 ? 1 : 0)) atomicOr(flags + f, kMultiRound);
    }
}

__global__ __launch_bounds__(kThreads) void converge_kernel(Geo g, const FrameDesc* __restrict__ desc, const int* __restrict__ skind,
                                                           const long long* __restrict__ isoff, const unsigned long long* __restrict__ st,
                                                           const unsigned long long* __restrict__ sin, int* __restrict__ flags) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.NS) return;
    const int f = frame_of<2>(desc, g.F, j);
    if (f < 0 || skind[j] < 0) return;
    const FrameDesc d = desc[f];
    if (!is_first(d, isoff, skind, j) && sin[j] != st[j - 1]) atomicOr(flags + f, kUnconverged);
}

// the exact backstop: one thread per restart interval of an unconverged frame
__global__ void serial_kernel(Geo g, const FrameDesc* __restrict__ desc, const unsigned char* __restrict__ tables,
                              const unsigned char* __restrict__ stream, const int* __restrict__ send, const long long* __restrict__ isoff,
                              unsigned long long* __restrict__ st, unsigned long long* __restrict__ sin, long long* __restrict__ cnt,
                              int* __restrict__ flags) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= g.NI) return;
    const int f = frame_of<1>(desc, g.F, k);
    if (f < 0 || !(flags[f] & kUnconverged) || (flags[f] & kCorrupt)) return;
    const FrameDesc d = desc[f];
    const Frame fr = frame_view(g, d, f, stream, tables);
    const long long j0 = d.sub_base + isoff[k] - isoff[d.int_base], j1 = d.sub_base + isoff[k + 1] - isoff[d.int_base];
    unsigned long long in = pack((int)(j0 - d.sub_base) * g.sub_bits, 0, 0);
    for (long long j = j0; j < min(j1, (long long)d.sub_base + d.sub_cap); ++j) {
        int p = st_p(in), c = st_c(in), z = st_z(in), err = 0;
        cnt[j] = decode_run<false>(fr, p, c, z, (int)(j - d.sub_base + 1) * g.sub_bits, send[j], err);
        sin[j] = in;
        in = pack(p, c, z);
        st[j] = in;
    }
    if (k == d.int_base) atomicOr(flags + f, kBackstop);
}

__global__ void block_check_kernel(Geo g, const FrameDesc* __restrict__ desc, const long long* __restrict__ isoff, const long long* __restrict__ boff,
                                   int* __restrict__ flags) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= g.NI) return;
    const int f = frame_of<1>(desc, g.F, k);
    if (f < 0) return;
    const FrameDesc d = desc[f];
    const int kk = (int)(k - d.int_base);
    const long long j0 = d.sub_base + isoff[k] - isoff[d.int_base], j1 = d.sub_base + isoff[k + 1] - isoff[d.int_base];
    if (j1 > (long long)d.sub_base + d.sub_cap) {
        atomicOr(flags + f, kCorrupt);
        return;
    }
    const long long want = (long long)min(d.ri, g.n_mcu - kk * d.ri) * g.bpm;
    if (boff[j1] - boff[j0] != want || boff[j0] - boff[d.sub_base] != (long long)kk * d.ri * g.bpm) atomicOr(flags + f, kCorrupt);
}

__global__ void zero_kernel(int4* __restrict__ p, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kThreads) void write_kernel(Geo g, const FrameDesc* __restrict__ desc, const unsigned char* __restrict__ tables,
                                                        const unsigned char* __restrict__ stream, const int* __restrict__ skind,
                                                        const int* __restrict__ send, const long long* __restrict__ isoff,
                                                        const unsigned long long* __restrict__ st, const long long* __restrict__ boff,
                                                        int* __restrict__ flags, int* __restrict__ dcdiff, short* __restrict__ coef) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.NS) return;
    const int f = frame_of<2>(desc, g.F, j);
    if (f < 0 || skind[j] < 0 || (flags[f] & kCorrupt)) return;
    const FrameDesc d = desc[f];
    const Frame fr = frame_view(g, d, f, stream, tables);
    const unsigned long long in = is_first(d, isoff, skind, j) ? pack((int)(j - d.sub_base) * g.sub_bits, 0, 0) : st[j - 1];
    int p = st_p(in), c = st_c(in), z = st_z(in), err = 0;
    const long long fb = (long long)f * g.nblk;
    decode_run<true>(fr, p, c, z, (int)(j - d.sub_base + 1) * g.sub_bits, send[j], err, boff[j] - boff[d.sub_base], g.nblk, dcdiff + fb,
                     coef + 64 * fb);
    if (err) atomicOr(flags + f, kCorrupt);
}

// ------------------------------------------------------------------------------------------------ DC prediction
__global__ __launch_bounds__(kThreads) void dc_kernel(Geo g, const FrameDesc* __restrict__ desc, const int* __restrict__ dcdiff,
                                                     short* __restrict__ coef) {
    __shared__ unsigned int sh_s[kThreads];
    __shared__ int sh_r[kThreads];
    const int f = blockIdx.x / g.nc, comp = blockIdx.x % g.nc, t = threadIdx.x;
    const int per = comp == 0 ? g.hs * g.vs : 1, off = comp == 0 ? 0 : g.hs * g.vs + comp - 1;
    const int ri = desc[f].ri > 0 ? desc[f].ri : g.n_mcu;
    const long long n = (long long)g.n_mcu * per, chunk = cdiv(n, kThreads), k0 = t * chunk, k1 = min(n, k0 + chunk);
    const long long fb = (long long)f * g.nblk;
    auto blk = [&](long long k) { return (k / per) * g.bpm + off + k % per; };
    auto resets = [&](long long k) { return k % per == 0 && (k / per) % ri == 0; };
    unsigned int s = 0;
    int r = 0;
    for (long long k = k0; k < k1; ++k) {
        if (resets(k)) {
            s = 0;
            r = 1;
        }
        s += (unsigned int)dcdiff[fb + blk(k)];
    }
    sh_s[t] = s;
    sh_r[t] = r;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {              // inclusive segmented scan: (a then b) = b.reset ? b : (a.s + b.s, a.reset)
        unsigned int ps = 0;
        int pr = 0;
        if (t >= o) {
            ps = sh_s[t - o];
            pr = sh_r[t - o];
        }
        __syncthreads();
        if (t >= o && !sh_r[t]) {
            sh_s[t] += ps;
            sh_r[t] = pr;
        }
        __syncthreads();
    }
    unsigned int run = t ? sh_s[t - 1] : 0u;
    for (long long k = k0; k < k1; ++k) {
        if (resets(k)) run = 0;
        run += (unsigned int)dcdiff[fb + blk(k)];
        coef[64 * (fb + blk(k))] = (short)(int)run;
    }
}

// ------------------------------------------------------------------------------------------------ IDCT (jidctint.c)
__device__ __forceinline__ long long descale(long long x, int n) { return (x + (1ll << (n - 1))) >> n; }

template <bool kPass1>
__device__ __forceinline__ void idct_1d(const long long* v, int s, long long* o, int os) {
    constexpr int n = kPass1 ? 13 - 2 : 13 + 2 + 3;
    long long z2 = v[2 * s], z3 = v[6 * s];
    long long z1 = (z2 + z3) * 4433;
    const long long tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
    const long long tmp0 = (v[0] + v[4 * s]) * 8192, tmp1 = (v[0] - v[4 * s]) * 8192;
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    long long t0 = v[7 * s], t1 = v[5 * s], t2 = v[3 * s], t3 = v[s];
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    long long z4 = t1 + t3;
    const long long z5 = (z3 + z4) * 9633;
    t0 *= 2446;
    t1 *= 16819;
    t2 *= 25172;
    t3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    o[0] = descale(tmp10 + t3, n);
    o[7 * os] = descale(tmp10 - t3, n);
    o[os] = descale(tmp11 + t2, n);
    o[6 * os] = descale(tmp11 - t2, n);
    o[2 * os] = descale(tmp12 + t1, n);
    o[5 * os] = descale(tmp12 - t1, n);
    o[3 * os] = descale(tmp13 + t0, n);
    o[4 * os] = descale(tmp13 - t0, n);
}

__global__ __launch_bounds__(kThreads) void idct_kernel(Geo g, const unsigned char* __restrict__ tables, const short* __restrict__ coef,
                                                       unsigned char* __restrict__ planes) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)g.F * g.nblk) return;
    const int f = (int)(i / g.nblk), b = (int)(i - (long long)f * g.nblk);
    const int m = b / g.bpm, cb = b - m * g.bpm, my = m / g.mw, mx = m - my * g.mw;
    const int ny = g.hs * g.vs;
    const int comp = cb < ny ? 0 : cb - ny + 1;
    const int h = comp ? 1 : g.hs, v = comp ? 1 : g.vs, a = comp ? 0 : cb / g.hs, bb = comp ? 0 : cb % g.hs;
    const unsigned char* blob = tables + (long long)f * kBlobBytes;
    const unsigned short* q = reinterpret_cast<const unsigned short*>(blob + kHdr) + 64 * (reinterpret_cast<const int*>(blob)[8 + comp] & 3);
    const short* cf = coef + 64 * i;
    long long x[64], ws[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) x[k] = (long long)cf[k] * (long long)(short)q[k];
#pragma unroll
    for (int col = 0; col < 8; ++col) idct_1d<true>(x + col, 8, ws + col, 8);
#pragma unroll
    for (int k = 0; k < 64; ++k) ws[k] = (long long)(int)ws[k];          // the int workspace
    unsigned char* pl = planes + (long long)f * g.pframe + g.poff[comp];
    const int pw = g.pw[comp];
    const long long y0 = (long long)(my * v + a) * 8, x0 = (long long)(mx * h + bb) * 8;
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        long long o[8];
        idct_1d<false>(ws + 8 * row, 1, o, 1);
        unsigned int w0 = 0, w1 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int vv = (int)(o[k] & 1023);
            if (vv >= 512) vv -= 1024;
            const unsigned int px = (unsigned int)min(max(vv + 128, 0), 255);
            if (k < 4) w0 |= px << (8 * k);
            else w1 |= px << (8 * (k - 4));
        }
        unsigned int* dstp = reinterpret_cast<unsigned int*>(pl + (y0 + row) * pw + x0);   // 8-byte aligned: pw and x0 are multiples of 8
        dstp[0] = w0;
        dstp[1] = w1;
    }
}

// ------------------------------------------------------------------------------------------------ upsampling and colour (jdsample.c, jdcolor.c)
__device__ __forceinline__ int chroma_at(const Geo& g, const unsigned char* pl, int pw, int y, int x) {
    if (g.hs == 1) return pl[(long long)y * pw + x];
    const int dw = (g.W + 1) >> 1, i = x >> 1;
    if (g.vs == 1) {                                                      // h2v1
        const unsigned char* r = pl + (long long)y * pw;
        const int s = r[i];
        if (dw <= 2) return s;
        if ((x & 1) == 0) return i == 0 ? s : (3 * s + r[i - 1] + 1) >> 2;
        return i == dw - 1 ? s : (3 * s + r[i + 1] + 2) >> 2;
    }
    const int dh = (g.H + 1) >> 1, ry = y >> 1;                           // h2v2
    if (dw <= 2) return pl[(long long)ry * pw + i];
    const int r2 = (y & 1) ? min(ry + 1, dh - 1) : max(ry - 1, 0);
    const unsigned char* r0 = pl + (long long)ry * pw;
    const unsigned char* r1 = pl + (long long)r2 * pw;
    const int cs = 3 * r0[i] + r1[i];
    if ((x & 1) == 0) return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
    return i == dw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
}

__device__ __forceinline__ unsigned int bgr_of(const Geo& g, const unsigned char* planes, long long pix) {
    const long long fhw = (long long)g.H * g.W;
    const int f = (int)(pix / fhw);
    const long long r = pix - f * fhw;
    const int y = (int)(r / g.W), x = (int)(r - (long long)y * g.W);
    const unsigned char* pf = planes + (long long)f * g.pframe;
    const int Y = pf[(long long)y * g.pw[0] + x];
    if (g.nc == 1) return (unsigned int)Y * 0x010101u;
    const int cb = chroma_at(g, pf + g.poff[1], g.pw[1], y, x) - 128, cr = chroma_at(g, pf + g.poff[2], g.pw[2], y, x) - 128;
    const int R = Y + ((91881 * cr + 32768) >> 16);
    const int G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int B = Y + ((116130 * cb + 32768) >> 16);
    return (unsigned int)min(max(B, 0), 255) | ((unsigned int)min(max(G, 0), 255) << 8) | ((unsigned int)min(max(R, 0), 255) << 16);
}

__global__ __launch_bounds__(kThreads) void color_kernel(Geo g, const unsigned char* __restrict__ planes, unsigned char* __restrict__ out, int aligned) {
    const long long n = (long long)g.F * g.H * g.W, i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    if (aligned && i + 4 <= n) {
        const unsigned int p0 = bgr_of(g, planes, i), p1 = bgr_of(g, planes, i + 1), p2 = bgr_of(g, planes, i + 2), p3 = bgr_of(g, planes, i + 3);
        unsigned int* o = reinterpret_cast<unsigned int*>(out + 3 * i);          // 12 bytes at a multiple of 12
        o[0] = p0 | (p1 << 24);
        o[1] = (p1 >> 8) | (p2 << 16);
        o[2] = (p2 >> 16) | (p3 << 8);
        return;
    }
    for (long long k = i; k < min(n, i + 4); ++k) {
        const unsigned int p = bgr_of(g, planes, k);
        out[3 * k] = (unsigned char)p;
        out[3 * k + 1] = (unsigned char)(p >> 8);
        out[3 * k + 2] = (unsigned char)(p >> 16);
    }
}

__global__ void status_kernel(int F, const int* __restrict__ flags, unsigned char* __restrict__ status) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) status[f] = (unsigned char)(flags[f] & (kCorrupt | kMultiRound | kBackstop));
}

int check_args(int F, int H, int W, int sampling, long long total_bytes, long long total_intervals, int sub_bits, int rounds, Geo& g, const char* who) {
    SS_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "%s: bad dims F=%d H=%d W=%d", who, F, H, W);
    SS_CHECK_ARG(total_bytes >= 0 && total_bytes < (1ll << 32) && total_intervals >= F, "%s: total_bytes=%lld total_intervals=%lld", who,
                 (long long)total_bytes, (long long)total_intervals);
    SS_CHECK_ARG(sub_bits == 0 || (sub_bits >= 64 && sub_bits % 64 == 0 && sub_bits <= 65536), "%s: sub_bits=%d (0, or a multiple of 64 in [64, 65536])",
                 who, sub_bits);
    SS_CHECK_ARG(rounds >= 0 && rounds <= 4096, "%s: max_rounds=%d", who, rounds);
    SS_CHECK_ARG(make_geo(F, H, W, sampling, total_bytes, total_intervals, sub_bits, rounds, g), "%s: sampling 0x%x is not 0, 0x11, 0x21 or 0x22",
                 who, sampling);
    SS_CHECK_ARG((long long)F * g.nblk < (1ll << 31) && g.NS < (1ll << 31) && g.NC < (1ll << 31) && total_intervals < (1ll << 31),
                 "%s: %d frames of %d x %d are too large for one call", who, F, H, W);
    return STEMSEG_OK;
}

}  // namespace

extern "C" size_t stemseg_hip_jpeg_decode_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t sampling, int64_t total_bytes,
                                                         int64_t total_intervals, int32_t sub_bits) {
    Geo g;
    if (check_args(F, H, W, sampling, total_bytes, total_intervals, sub_bits, 0, g, "jpeg_decode_workspace_bytes") != STEMSEG_OK) return 0;
    return layout(nullptr, g).bytes;
}

extern "C" int stemseg_hip_jpeg_decode(const uint8_t* data, const int64_t* ecs_offsets, const uint8_t* tables, int32_t F, int32_t H, int32_t W,
                                       int32_t sampling, int64_t total_bytes, int64_t total_intervals, int32_t sub_bits, int32_t max_rounds,
                                       void* workspace, size_t ws_bytes, uint8_t* out, uint8_t* status, void* stream) {
    Geo g;
    int rc = check_args(F, H, W, sampling, total_bytes, total_intervals, sub_bits, max_rounds, g, "jpeg_decode");
    if (rc != STEMSEG_OK) return rc;
    SS_CHECK_ARG(data && ecs_offsets && tables && workspace && out && status, "jpeg_decode: null pointer");
    Ws w = layout(static_cast<char*>(workspace), g);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "jpeg_decode: workspace %zu bytes < %zu", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const long long NB = (long long)F * g.nblk;
    hipLaunchKernelGGL(setup_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const long long*>(ecs_offsets), tables, g, w.desc, w.flags);
    hipLaunchKernelGGL(interval_init_kernel, dim3(grid(g.NI)), dim3(kThreads), 0, s, g, w.istart);
    hipLaunchKernelGGL(chunk_count_kernel, dim3(grid(g.NC)), dim3(kThreads), 0, s, data, g, w.desc, w.flags, w.ccnt);
    launch_scan(w.ccnt, nullptr, g.NC, w.tile_sums, w.coff, s);
    hipLaunchKernelGGL(rst_kernel, dim3(grid(g.NC)), dim3(kThreads), 0, s, data, g, w.desc, w.coff, w.flags, w.istart);
    hipLaunchKernelGGL(interval_len_kernel, dim3(grid(g.NI)), dim3(kThreads), 0, s, g, w.desc, w.coff, w.istart, w.flags, w.ilen, w.isubs);
    launch_scan(w.isubs, nullptr, g.NI, w.tile_sums, w.isoff, s);
    hipLaunchKernelGGL(scatter_kernel, dim3(grid(g.NC)), dim3(kThreads), 0, s, data, g, w.desc, w.coff, w.istart, w.ilen, w.isoff, w.stream);
    hipLaunchKernelGGL(sub_info_kernel, dim3(grid(g.NS)), dim3(kThreads), 0, s, g, w.desc, w.ilen, w.isoff, w.flags, w.skind, w.send);
    hipLaunchKernelGGL(spec_kernel, dim3(grid(g.NS)), dim3(kThreads), 0, s, g, w.desc, tables, w.stream, w.skind, w.send, w.st[0], w.sin, w.cnt);
    for (int l = 0; l < kSyncLaunches; ++l)
        hipLaunchKernelGGL(sync_kernel, dim3(g.NS / kThreads), dim3(kThreads), 0, s, g, l, w.desc, tables, w.stream, w.skind, w.send, w.isoff,
                           w.st[l & 1], w.st[(l + 1) & 1], w.sin, w.cnt, w.flags);
    unsigned long long* fin = w.st[kSyncLaunches & 1];
    hipLaunchKernelGGL(converge_kernel, dim3(grid(g.NS)), dim3(kThreads), 0, s, g, w.desc, w.skind, w.isoff, fin, w.sin, w.flags);
    hipLaunchKernelGGL(serial_kernel, dim3(grid(g.NI)), dim3(kThreads), 0, s, g, w.desc, tables, w.stream, w.send, w.isoff, fin, w.sin, w.cnt,
                       w.flags);
    launch_scan(w.cnt, nullptr, g.NS, w.tile_sums, w.boff, s);
    hipLaunchKernelGGL(block_check_kernel, dim3(grid(g.NI)), dim3(kThreads), 0, s, g, w.desc, w.isoff, w.boff, w.flags);
    hipLaunchKernelGGL(zero_kernel, dim3(std::min(grid(NB * 8), 4096)), dim3(kThreads), 0, s, reinterpret_cast<int4*>(w.coef), NB * 8);
    hipLaunchKernelGGL(write_kernel, dim3(grid(g.NS)), dim3(kThreads), 0, s, g, w.desc, tables, w.stream, w.skind, w.send, w.isoff, fin, w.boff,
                       w.flags, w.dcdiff, w.coef);
    hipLaunchKernelGGL(dc_kernel, dim3(F * g.nc), dim3(kThreads), 0, s, g, w.desc, w.dcdiff, w.coef);
    hipLaunchKernelGGL(idct_kernel, dim3(grid(NB)), dim3(kThreads), 0, s, g, tables, w.coef, w.planes);
    const long long npx = (long long)F * H * W;
    hipLaunchKernelGGL(color_kernel, dim3(grid(cdiv(npx, 4))), dim3(kThreads), 0, s, g, w.planes, out,
                       (int)((reinterpret_cast<uintptr_t>(out) & 3) == 0));
    hipLaunchKernelGGL(status_kernel, dim3(grid(F)), dim3(kThreads), 0, s, F, w.flags, status);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
