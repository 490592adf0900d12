// Device half of the save_vis visualisations (output_utils/davis.py:124-161, youtube_vis.py:193-222, kitti_mots.py:208-239).
//
// (1) Overlay composite of a condensed index map M[F][H][W] (uint8 / uint16, value n = kept instance n, 0 = none) on BGR frames:
//     a pixel with 1 <= n <= K gets trunc(0.6 * colors[n][c] + (1 - 0.6) * img[c]) per channel c -- utils/vis.py
//     overlay_mask_on_image as numpy evaluates it (two separately rounded fp64 products, an fp64 add, astype(uint8)); the
//     palette's R, G, B go to channels 0, 1, 2 of the BGR image, as the reference applies its RGB map to cv2's image.  Every other
//     pixel is copied (0.6 * s + 0.4 * s truncates back to s for every uint8 s).
// (2) Baseline JFIF encoder, byte-identical to libjpeg-turbo as PIL drives it (quality q, 4:2:0, standard Huffman tables, no
//     restart markers) and so to cv2.imwrite's defaults.  F frames of one size per call:
//       fdct    : one thread per (frame, MCU, block) -- Y0 Y1 Y2 Y3 Cb Cr -- converts RGB -> YCbCr (jccolor fixed point), downsamples
//                 h2v2 with the alternating bias (jcsample), replicates the edges as jcprepct does, runs the islow FDCT
//                 (jfdctint), quantises with the reciprocal of the 16-bit SIMD build (jcdctmgr), writes zigzag int16 coefficients
//                 and the bit length of the AC codes.  Blocks right of / below the image are dummies (jccoefct): zero AC
//       dc      : resolves every block's DC (a dummy carries its neighbour's quantised DC) and adds the DC-difference length,
//                 predicted per component in coding order
//       scans   : block bit lengths -> bit offsets; per-frame word counts -> word-aligned frame bases
//       emit    : one thread per block packs its codes MSB-first at its bit offset; words that straddle two blocks take
//                 atomicOr (same bits in any order), the last block of a frame pads with 1 bits to a byte boundary
//       ffcount : 0xFF bytes per 256-byte chunk of a frame, scanned; frame file sizes, scanned
//     The plan call stops there and reports the per-frame file sizes; the encode call writes each file (header, the entropy-coded
//     data with 0x00 stuffed after every 0xFF, EOI) and the file offsets.  A fixed launch count whatever F or the data.
#include "common.h"
#include "scan.h"

#include <algorithm>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 256;                       // bytes per stuffing chunk
constexpr int kMaxBlockBits = 27 + 63 * 26;       // DC code + value (16 + 11) and 63 AC codes + values (16 + 10)

int grid_for(long long n, int cap) { return (int)std::max<long long>(1, std::min<long long>(ceil_div(n, kThreads), cap)); }

// ------------------------------------------------------------------------------------------------ composite
template <typename IdxT>
__global__ void composite_kernel(const unsigned char* __restrict__ frames, const IdxT* __restrict__ maps, long long n_px,
                                 const unsigned char* __restrict__ colors, int K, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)                         // numpy rounds both products: no fma (__dmul_rn / __dadd_rn would still fuse)
    const double wc = 0.6, wi = 1.0 - 0.6;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (long long)gridDim.x * blockDim.x) {
        const unsigned int n = maps[i];
        const unsigned char* px = frames + 3 * i;
        unsigned char* o = out + 3 * i;
        if (n >= 1 && n <= (unsigned int)K) {
            const unsigned char* c = colors + 3 * n;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                o[ch] = (unsigned char)(int)(wc * (double)c[ch] + wi * (double)px[ch]);
        } else {
            o[0] = px[0];
            o[1] = px[1];
            o[2] = px[2];
        }
    }
}

// ------------------------------------------------------------------------------------------------ tables (ITU T.81 Annex K)
struct HuffTab {
    unsigned short code[256];
    unsigned char len[256];
};

constexpr HuffTab make_tab(const unsigned char (&bits)[16], const unsigned char* vals) {
    HuffTab t{};
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i) {
            t.code[vals[k]] = (unsigned short)code;
            t.len[vals[k]] = (unsigned char)l;
            ++code;
            ++k;
        }
        code <<= 1;
    }
    return t;
}

constexpr unsigned char kDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char kDcBitsC[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr unsigned char kAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char kAcBitsC[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr unsigned char kAcValsC[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char kLumaQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                        47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr unsigned char kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                                       7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                       39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__constant__ HuffTab kDcTab[2] = {make_tab(kDcBits, kDcVals), make_tab(kDcBitsC, kDcVals)};
__constant__ HuffTab kAcTab[2] = {make_tab(kAcBits, kAcVals), make_tab(kAcBitsC, kAcValsC)};
__constant__ unsigned char kZz[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                                      7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                      39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// quality -> reciprocal quantiser of both tables (jcparam jpeg_quality_scaling + jpeg_add_quant_table with force_baseline, then
// jcdctmgr compute_reciprocal for divisor 8 * q with a 16-bit DCTELEM): |x| -> ((|x| + corr) * recip) >> (16 + shift)
struct Quant {
    unsigned short recip[2][64];
    unsigned short corr[2][64];
    unsigned char shift[2][64];
    unsigned char table[2][64];          // natural order, for the DQT markers
};

Quant make_quant(int quality) {
    Quant q{};
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = std::min(std::max(((t ? kChromaQ : kLumaQ)[i] * scale + 50) / 100, 1), 255);
            q.table[t][i] = (unsigned char)v;
            const unsigned int d = 8u * v;
            int b = 0;
            while ((d >> (b + 1)) != 0) ++b;
            int r = 16 + b;
            unsigned int fq = (1u << r) / d, fr = (1u << r) % d, c = d / 2;
            if (fr == 0) {
                fq >>= 1;
                --r;
            } else if (fr <= d / 2) {
                ++c;
            } else {
                ++fq;
            }
            q.recip[t][i] = (unsigned short)fq;
            q.corr[t][i] = (unsigned short)c;
            q.shift[t][i] = (unsigned char)(r - 16);
        }
    return q;
}

constexpr int kMaxHeader = 640;
struct Header {
    unsigned char b[kMaxHeader];
    int len;
};

// SOI, JFIF 1.01 APP0 (density 1:1, unit 0), DQT x2, SOF0 (Y 2x2, Cb / Cr 1x1), DHT x4 (DC0 AC0 DC1 AC1), SOS: as jcmarker writes it
Header make_header(int H, int W, const Quant& q) {
    Header h{};
    int n = 0;
    auto put = [&](int v) { h.b[n++] = (unsigned char)v; };
    auto marker = [&](int m, int payload) { put(0xFF); put(m); put((payload + 2) >> 8); put((payload + 2) & 255); };
    put(0xFF); put(0xD8);
    marker(0xE0, 14);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);   // "JFIF\0", 1.01, unit 0, 1:1, no thumbnail
    for (int t = 0; t < 2; ++t) {
        marker(0xDB, 65);
        put(t);
        for (int k = 0; k < 64; ++k) put(q.table[t][kZigzag[k]]);
    }
    marker(0xC0, 15);
    for (int v : {8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);
    const unsigned char* bits[4] = {kDcBits, kAcBits, kDcBitsC, kAcBitsC};
    const unsigned char* vals[4] = {kDcVals, kAcVals, kDcVals, kAcValsC};
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        int nv = 0;
        for (int l = 0; l < 16; ++l) nv += bits[t][l];
        marker(0xC4, 17 + nv);
        put(ids[t]);
        for (int l = 0; l < 16; ++l) put(bits[t][l]);
        for (int i = 0; i < nv; ++i) put(vals[t][i]);
    }
    marker(0xDA, 10);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) put(v);
    h.len = n;
    return h;
}

// ------------------------------------------------------------------------------------------------ geometry and workspace
struct Geo {
    int H, W, mh, mw, hib, wib, nblk;      // MCU rows / columns, Y blocks high / wide inside the image, blocks per frame
    long long words_per_frame, chunks_per_frame;
};

Geo make_geo(int H, int W) {
    Geo g;
    g.H = H;
    g.W = W;
    g.mh = (int)ceil_div(H, 16);
    g.mw = (int)ceil_div(W, 16);
    g.hib = (int)ceil_div(H, 8);
    g.wib = (int)ceil_div(W, 8);
    g.nblk = g.mh * g.mw * 6;
    g.words_per_frame = ceil_div((long long)g.nblk * kMaxBlockBits + 7, 32);
    g.chunks_per_frame = ceil_div(4 * g.words_per_frame, kChunk);
    return g;
}

struct JpegWs {
    short* coef;                 // [NB][64] zigzag
    int* dc;                     // [NB] quantised DC of the real blocks
    long long* bits;             // [NB] block bit lengths
    long long* bitoff;           // [NB + 1]
    long long* fwords;           // [F] words of each frame's entropy-coded data
    long long* wbase;            // [F + 1]
    unsigned int* words;         // [F * words_per_frame] the packed bits
    long long* ffcnt;            // [F * chunks_per_frame] 0xFF bytes per chunk
    long long* ffoff;            // [F * chunks_per_frame + 1]
    long long* fbytes;           // [F] file sizes
    long long* foff;             // [F + 1] file offsets
    long long* tile_sums;
    size_t bytes;
};

JpegWs jpeg_layout(char* base, int F, const Geo& g) {
    JpegWs w{};
    size_t o = 0;
    auto take = [&](size_t n) { void* p = base ? base + o : nullptr; o += round_up((long long)n, 256); return p; };
    const long long NB = (long long)F * g.nblk, NC = (long long)F * g.chunks_per_frame;
    w.coef = (short*)take(2 * 64 * NB);
    w.dc = (int*)take(4 * NB);
    w.bits = (long long*)take(8 * NB);
    w.bitoff = (long long*)take(8 * (NB + 1));
    w.fwords = (long long*)take(8 * F);
    w.wbase = (long long*)take(8 * (F + 1));
    w.words = (unsigned int*)take(4 * F * g.words_per_frame);
    w.ffcnt = (long long*)take(8 * NC);
    w.ffoff = (long long*)take(8 * (NC + 1));
    w.fbytes = (long long*)take(8 * F);
    w.foff = (long long*)take(8 * (F + 1));
    w.tile_sums = (long long*)take(8 * (scan_tiles(std::max<long long>(NB, NC)) + 1));
    w.bytes = o;
    return w;
}

// ------------------------------------------------------------------------------------------------ samples
__device__ __forceinline__ void rgb_at(const unsigned char* fr, int W, int y, int x, int& r, int& g, int& b) {
    const unsigned char* p = fr + 3 * ((long long)y * W + x);
    b = p[0];
    g = p[1];
    r = p[2];
}

// jccolor rgb_ycc_convert, FIX(x) = (int)(x * 65536 + 0.5)
__device__ __forceinline__ int y_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int cb_of(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int cr_of(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

__device__ __forceinline__ long long descale(long long v, int n) { return (v + (1ll << (n - 1))) >> n; }

// jfdctint.c jpeg_fdct_islow on 8 values at stride s (pass 1: rows, output scaled up by 4; pass 2: columns, scaled down by 4)
template <bool kPass1>
__device__ __forceinline__ void fdct_1d(long long* d, int s) {
    const long long tmp0 = d[0] + d[7 * s], tmp7 = d[0] - d[7 * s];
    const long long tmp1 = d[s] + d[6 * s], tmp6 = d[s] - d[6 * s];
    const long long tmp2 = d[2 * s] + d[5 * s], tmp5 = d[2 * s] - d[5 * s];
    const long long tmp3 = d[3 * s] + d[4 * s], tmp4 = d[3 * s] - d[4 * s];
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int n = kPass1 ? 13 - 2 : 13 + 2;
    if (kPass1) {
        d[0] = (tmp10 + tmp11) * 4;
        d[4 * s] = (tmp10 - tmp11) * 4;
    } else {
        d[0] = descale(tmp10 + tmp11, 2);
        d[4 * s] = descale(tmp10 - tmp11, 2);
    }
    long long z1 = (tmp12 + tmp13) * 4433;
    d[2 * s] = descale(z1 + tmp13 * 6270, n);
    d[6 * s] = descale(z1 - tmp12 * 15137, n);
    z1 = tmp4 + tmp7;
    long long z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const long long z5 = (z3 + z4) * 9633;
    const long long t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * s] = descale(t4 + z1 + z3, n);
    d[5 * s] = descale(t5 + z2 + z4, n);
    d[3 * s] = descale(t6 + z2 + z3, n);
    d[s] = descale(t7 + z1 + z4, n);
}

// block j (0..5) of MCU (my, mx) lies inside the image (not a dummy)
__device__ __forceinline__ bool real_block(const Geo& g, int my, int mx, int j) {
    if (j >= 4) return true;
    return 2 * my + (j >> 1) < g.hib && 2 * mx + (j & 1) < g.wib;
}

__device__ __forceinline__ int bit_len(int v) { return v ? 32 - __clz(v) : 0; }

__global__ __launch_bounds__(kThreads) void jpeg_fdct_kernel(const unsigned char* __restrict__ frames, int F, Geo g, Quant q,
                                                             short* __restrict__ coef, int* __restrict__ dc, long long* __restrict__ bits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * g.nblk) return;
    const int f = (int)(i / g.nblk), rem = (int)(i - (long long)f * g.nblk);
    const int m = rem / 6, j = rem - 6 * m, my = m / g.mw, mx = m - my * g.mw;
    short* out = coef + 64 * i;
    const int t = j >= 4;
    if (!real_block(g, my, mx, j)) {          // dummy: zero AC, an EOB; the DC pass fills its DC
        for (int k = 0; k < 64; ++k) out[k] = 0;
        bits[i] = kAcTab[0].len[0];
        return;
    }
    const unsigned char* fr = frames + (long long)f * g.H * g.W * 3;
    long long d[64];
    if (!t) {
        const int y0 = 16 * my + 8 * (j >> 1), x0 = 16 * mx + 8 * (j & 1);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int y = min(y0 + r, g.H - 1);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                int R, G, B;
                rgb_at(fr, g.W, y, min(x0 + c, g.W - 1), R, G, B);
                d[8 * r + c] = y_of(R, G, B) - 128;
            }
        }
    } else {
        // rows go in pairs (an odd last row pairs with itself), downsampled rows past the last pair repeat it; columns replicate
        // the right edge at full resolution; bias 1, 2, 1, 2, ... along each downsampled row
        const int n_pairs = (g.H + 1) / 2;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int pr = min(8 * my + r, n_pairs - 1), r0 = 2 * pr, r1 = min(2 * pr + 1, g.H - 1);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int cx = 8 * mx + c, c0 = min(2 * cx, g.W - 1), c1 = min(2 * cx + 1, g.W - 1);
                const int ys[2] = {r0, r1}, xs[2] = {c0, c1};
                int s = 0;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        int R, G, B;
                        rgb_at(fr, g.W, ys[a], xs[b], R, G, B);
                        s += j == 4 ? cb_of(R, G, B) : cr_of(R, G, B);
                    }
                d[8 * r + c] = ((s + 1 + (cx & 1)) >> 2) - 128;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_1d<true>(d + 8 * r, 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_1d<false>(d + c, 8);
    long long nb = 0;
    int run = 0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int nat = kZz[k];
        const long long x = d[nat];
        const unsigned int a = (unsigned int)(x < 0 ? -x : x);
        const int qa = (int)(((a + q.corr[t][nat]) * (unsigned int)q.recip[t][nat]) >> (16 + q.shift[t][nat]));
        const int v = x < 0 ? -qa : qa;
        out[k] = (short)v;
        if (k == 0) {
            dc[i] = v;
            continue;
        }
        if (v == 0) {
            ++run;
            continue;
        }
        nb += (run >> 4) * kAcTab[t].len[0xF0];
        run &= 15;
        const int l = bit_len(qa);
        nb += kAcTab[t].len[(run << 4) + l] + l;
        run = 0;
    }
    if (run) nb += kAcTab[t].len[0];
    bits[i] = nb;
}

// the quantised DC of block j of MCU m (dummies: right -> the left neighbour, bottom row -> block Y1 of the MCU)
__device__ __forceinline__ int dc_of(const Geo& g, const int* dc_frame, int m, int j) {
    const int my = m / g.mw, mx = m - my * g.mw;
    if (j < 4 && 2 * my + (j >> 1) >= g.hib) j = 1;
    if (j < 4 && 2 * mx + (j & 1) >= g.wib) j -= 1;
    return dc_frame[6 * m + j];
}

__global__ __launch_bounds__(kThreads) void jpeg_dc_kernel(int F, Geo g, const int* __restrict__ dc, short* __restrict__ coef,
                                                           long long* __restrict__ bits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * g.nblk) return;
    const int f = (int)(i / g.nblk), rem = (int)(i - (long long)f * g.nblk);
    const int m = rem / 6, j = rem - 6 * m;
    const int* dcf = dc + (long long)f * g.nblk;
    const int v = dc_of(g, dcf, m, j);
    int pred = 0;                                            // the previous block of the same component in coding order
    if (j >= 1 && j <= 3) pred = dc_of(g, dcf, m, j - 1);
    else if (m > 0) pred = dc_of(g, dcf, m - 1, j == 0 ? 3 : j);
    coef[64 * i] = (short)v;
    const int diff = v - pred, l = bit_len(diff < 0 ? -diff : diff);
    bits[i] += kDcTab[j >= 4].len[l] + l;
}

__global__ void jpeg_frame_words_kernel(int F, int nblk, const long long* __restrict__ bitoff, long long* __restrict__ fwords) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const long long fb = bitoff[(long long)(f + 1) * nblk] - bitoff[(long long)f * nblk];
    fwords[f] = (fb + 31) >> 5;
}

__global__ void jpeg_zero_kernel(unsigned int* __restrict__ words, const long long* __restrict__ n_dev) {
    const long long n = *n_dev;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) words[i] = 0u;
}

// MSB-first bit writer at an absolute bit position; every word it touches takes an atomicOr.  `lim` (the end of the word buffer)
// range) is never reached by a valid block; it only keeps a corrupt one inside the workspace.
struct BitSink {
    unsigned int* words;
    long long wi, lim;
    unsigned long long acc;      // left-aligned: bit 63 is the first bit of word wi
    int fill;

    __device__ void put(unsigned int code, int len) {
        if (!len) return;
        acc |= (unsigned long long)(code & ((1u << len) - 1u)) << (64 - fill - len);
        fill += len;
        while (fill >= 32) {
            if (wi < lim) atomicOr(words + wi, (unsigned int)(acc >> 32));
            acc <<= 32;
            fill -= 32;
            ++wi;
        }
    }
    __device__ void flush() {
        if (fill && wi < lim) atomicOr(words + wi, (unsigned int)(acc >> 32));
    }
};

__global__ __launch_bounds__(kThreads) void jpeg_emit_kernel(int F, Geo g, const short* __restrict__ coef, const long long* __restrict__ bitoff,
                                                             const long long* __restrict__ wbase, unsigned int* __restrict__ words) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * g.nblk) return;
    const int f = (int)(i / g.nblk), rem = (int)(i - (long long)f * g.nblk);
    const int m = rem / 6, j = rem - 6 * m, t = j >= 4;
    const long long* fo = bitoff + (long long)f * g.nblk;
    const long long pos = 32 * wbase[f] + (bitoff[i] - fo[0]);
    BitSink bs{words, pos >> 5, (long long)F * g.words_per_frame, 0ull, (int)(pos & 31)};
    const short* b = coef + 64 * i;
    int pred = 0;                                            // the DC pass left every block's resolved DC in coef[0]
    if (j >= 1 && j <= 3) pred = b[-64];
    else if (m > 0) pred = j == 0 ? b[-3 * 64] : b[-6 * 64];
    const int diff = b[0] - pred, l = bit_len(diff < 0 ? -diff : diff);
    bs.put(kDcTab[t].code[l], kDcTab[t].len[l]);
    bs.put((unsigned int)(diff < 0 ? diff - 1 : diff), l);
    const HuffTab& ac = kAcTab[t];
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = b[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) bs.put(ac.code[0xF0], ac.len[0xF0]);
        const int n = bit_len(v < 0 ? -v : v);
        bs.put(ac.code[(run << 4) + n], ac.len[(run << 4) + n]);
        bs.put((unsigned int)(v < 0 ? v - 1 : v), n);
        run = 0;
    }
    if (run) bs.put(ac.code[0], ac.len[0]);
    if (rem == g.nblk - 1) {                                 // last block of the frame: pad the last byte with 1 bits
        const int pad = (int)((8 - ((fo[g.nblk] - fo[0]) & 7)) & 7);
        bs.put((1u << pad) - 1u, pad);
    }
    bs.flush();
}

__device__ __forceinline__ unsigned int byte_at(const unsigned int* w, long long k) { return (w[k >> 2] >> (24 - 8 * (k & 3))) & 255u; }

__device__ __forceinline__ long long frame_data_bytes(const long long* bitoff, int nblk, int f) {
    return (bitoff[(long long)(f + 1) * nblk] - bitoff[(long long)f * nblk] + 7) >> 3;
}

__global__ __launch_bounds__(kThreads) void jpeg_ffcount_kernel(int F, Geo g, const long long* __restrict__ bitoff, const long long* __restrict__ wbase,
                                                                const unsigned int* __restrict__ words, long long* __restrict__ ffcnt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * g.chunks_per_frame) return;
    const int f = (int)(i / g.chunks_per_frame);
    const long long c = i - (long long)f * g.chunks_per_frame;
    const long long n = frame_data_bytes(bitoff, g.nblk, f);
    const unsigned int* w = words + wbase[f];
    long long cnt = 0;
    for (long long k = c * kChunk, e = min(n, (c + 1) * kChunk); k < e; ++k) cnt += byte_at(w, k) == 255u;
    ffcnt[i] = cnt;
}

__global__ void jpeg_frame_bytes_kernel(int F, Geo g, int hdr_len, const long long* __restrict__ bitoff, const long long* __restrict__ ffoff,
                                        long long* __restrict__ fbytes, long long* __restrict__ out_bytes) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const long long c0 = (long long)f * g.chunks_per_frame;
    const long long v = hdr_len + frame_data_bytes(bitoff, g.nblk, f) + (ffoff[c0 + g.chunks_per_frame] - ffoff[c0]) + 2;
    fbytes[f] = v;
    out_bytes[f] = v;
}

__global__ void jpeg_total_kernel(int F, const long long* __restrict__ foff, long long* __restrict__ total) { *total = foff[F]; }

// ------------------------------------------------------------------------------------------------ encode: the files
__global__ __launch_bounds__(kThreads) void jpeg_copy_kernel(int F, Geo g, int hdr_len, const long long* __restrict__ bitoff,
                                                             const long long* __restrict__ wbase, const unsigned int* __restrict__ words,
                                                             const long long* __restrict__ ffoff, const long long* __restrict__ foff,
                                                             unsigned char* __restrict__ out, long long cap) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * g.chunks_per_frame) return;
    const int f = (int)(i / g.chunks_per_frame);
    const long long c = i - (long long)f * g.chunks_per_frame;
    const long long n = frame_data_bytes(bitoff, g.nblk, f);
    if (c * kChunk >= n) return;
    const unsigned int* w = words + wbase[f];
    long long o = foff[f] + hdr_len + c * kChunk + (ffoff[i] - ffoff[(long long)f * g.chunks_per_frame]);
    const long long end = min(foff[f + 1] - 2, cap);
    for (long long k = c * kChunk, e = min(n, (c + 1) * kChunk); k < e; ++k) {
        const unsigned int v = byte_at(w, k);
        if (o < end) out[o] = (unsigned char)v;
        ++o;
        if (v == 255u) {
            if (o < end) out[o] = 0;
            ++o;
        }
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_header_kernel(int F, Header hdr, const long long* __restrict__ foff, unsigned char* __restrict__ out,
                                                               long long cap, long long* __restrict__ offsets) {
    const int f = blockIdx.x;
    const long long o = foff[f], e = foff[f + 1];
    for (int k = threadIdx.x; k < hdr.len; k += blockDim.x)
        if (o + k < min(e, cap)) out[o + k] = hdr.b[k];
    if (threadIdx.x == 0) {
        if (e <= cap && e - 2 >= o + hdr.len) {
            out[e - 2] = 0xFF;
            out[e - 1] = 0xD9;
        }
        offsets[f] = o;
        if (f == F - 1) offsets[F] = e;
    }
}

int check_jpeg_args(const void* p, int F, int H, int W, int quality, const char* who) {
    SS_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: bad dims F=%d H=%d W=%d", who, F, H, W);
    SS_CHECK_ARG(H <= 65535 && W <= 65535, "%s: a JPEG frame is at most 65535 x 65535, got %d x %d", who, H, W);
    SS_CHECK_ARG((long long)F * ceil_div(H, 16) * ceil_div(W, 16) * 6 < (1ll << 31), "%s: %d frames of %d x %d exceed 2^31 blocks", who, F, H, W);
    SS_CHECK_ARG(quality >= 1 && quality <= 100, "%s: quality must be in [1, 100], got %d", who, quality);
    SS_CHECK_ARG(p != nullptr, "%s: null pointer", who);
    return STEMSEG_OK;
}

}  // namespace

extern "C" int stemseg_hip_vis_composite(const uint8_t* frames, const void* index_map, int32_t index_bytes, int32_t F, int32_t H, int32_t W,
                                         const uint8_t* colors, int32_t K, uint8_t* out, void* stream) {
    SS_CHECK_ARG(index_bytes == 1 || index_bytes == 2, "vis_composite: index_bytes must be 1 or 2, got %d", index_bytes);
    SS_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && K >= 0, "vis_composite: bad dims F=%d H=%d W=%d K=%d", F, H, W, K);
    SS_CHECK_ARG(K <= (index_bytes == 1 ? 255 : 65535), "vis_composite: K=%d does not fit %d-byte indices", K, index_bytes);
    SS_CHECK_ARG(frames && index_map && colors && out, "vis_composite: null pointer");
    hipStream_t s = as_stream(stream);
    const long long n = (long long)F * H * W;
    if (index_bytes == 1)
        hipLaunchKernelGGL(composite_kernel<unsigned char>, dim3(grid_for(n, 8192)), dim3(kThreads), 0, s, frames,
                           static_cast<const unsigned char*>(index_map), n, colors, K, out);
    else
        hipLaunchKernelGGL(composite_kernel<unsigned short>, dim3(grid_for(n, 8192)), dim3(kThreads), 0, s, frames,
                           static_cast<const unsigned short*>(index_map), n, colors, K, out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_jpeg_workspace_bytes(int32_t F, int32_t H, int32_t W) {
    if (F < 1 || H < 1 || W < 1 || H > 65535 || W > 65535) return 0;
    return jpeg_layout(nullptr, F, make_geo(H, W)).bytes;
}

extern "C" int stemseg_hip_jpeg_plan(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t quality, void* workspace, size_t ws_bytes,
                                     int64_t* frame_bytes, int64_t* total, void* stream) {
    int rc = check_jpeg_args(frames, F, H, W, quality, "jpeg_plan");
    if (rc != STEMSEG_OK) return rc;
    SS_CHECK_ARG(workspace && frame_bytes && total, "jpeg_plan: null pointer");
    const Geo g = make_geo(H, W);
    JpegWs w = jpeg_layout(static_cast<char*>(workspace), F, g);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "jpeg_plan: workspace %zu bytes < %zu", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const Quant q = make_quant(quality);
    const int hdr_len = make_header(H, W, q).len;
    const long long NB = (long long)F * g.nblk, NC = (long long)F * g.chunks_per_frame;
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3(ceil_div(NB, kThreads)), dim3(kThreads), 0, s, frames, F, g, q, w.coef, w.dc, w.bits);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(ceil_div(NB, kThreads)), dim3(kThreads), 0, s, F, g, w.dc, w.coef, w.bits);
    launch_scan(w.bits, nullptr, NB, w.tile_sums, w.bitoff, s);
    hipLaunchKernelGGL(jpeg_frame_words_kernel, dim3(ceil_div(F, kThreads)), dim3(kThreads), 0, s, F, g.nblk, w.bitoff, w.fwords);
    launch_scan(w.fwords, nullptr, F, w.tile_sums, w.wbase, s);
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(grid_for((long long)F * g.words_per_frame, 4096)), dim3(kThreads), 0, s, w.words, w.wbase + F);
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3(ceil_div(NB, kThreads)), dim3(kThreads), 0, s, F, g, w.coef, w.bitoff, w.wbase, w.words);
    hipLaunchKernelGGL(jpeg_ffcount_kernel, dim3(ceil_div(NC, kThreads)), dim3(kThreads), 0, s, F, g, w.bitoff, w.wbase, w.words, w.ffcnt);
    launch_scan(w.ffcnt, nullptr, NC, w.tile_sums, w.ffoff, s);
    hipLaunchKernelGGL(jpeg_frame_bytes_kernel, dim3(ceil_div(F, kThreads)), dim3(kThreads), 0, s, F, g, hdr_len, w.bitoff, w.ffoff, w.fbytes,
                       reinterpret_cast<long long*>(frame_bytes));
    launch_scan(w.fbytes, nullptr, F, w.tile_sums, w.foff, s);
    hipLaunchKernelGGL(jpeg_total_kernel, dim3(1), dim3(1), 0, s, F, w.foff, reinterpret_cast<long long*>(total));
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_jpeg_encode(int32_t F, int32_t H, int32_t W, int32_t quality, void* workspace, size_t ws_bytes, uint8_t* out,
                                       int64_t out_bytes, int64_t* offsets, void* stream) {
    int rc = check_jpeg_args(workspace, F, H, W, quality, "jpeg_encode");
    if (rc != STEMSEG_OK) return rc;
    SS_CHECK_ARG(out && offsets, "jpeg_encode: null pointer");
    SS_CHECK_ARG(out_bytes >= 1, "jpeg_encode: out_bytes=%lld", (long long)out_bytes);
    const Geo g = make_geo(H, W);
    JpegWs w = jpeg_layout(static_cast<char*>(workspace), F, g);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "jpeg_encode: workspace %zu bytes < %zu", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    const Header hdr = make_header(H, W, make_quant(quality));
    const long long NC = (long long)F * g.chunks_per_frame;
    hipLaunchKernelGGL(jpeg_copy_kernel, dim3(ceil_div(NC, kThreads)), dim3(kThreads), 0, s, F, g, hdr.len, w.bitoff, w.wbase, w.words, w.ffoff,
                       w.foff, out, (long long)out_bytes);
    hipLaunchKernelGGL(jpeg_header_kernel, dim3(F), dim3(kThreads), 0, s, F, hdr, w.foff, out, (long long)out_bytes,
                       reinterpret_cast<long long*>(offsets));
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
