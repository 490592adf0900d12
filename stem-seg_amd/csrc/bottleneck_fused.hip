// Back-to-back GEMM for the bottleneck tail (f16x3 mode): conv3 of block b (1x1, MID -> 4 MID, + bias + identity + ReLU) and conv1 of
// block b + 1 (1x1, 4 MID -> MID, + bias + ReLU) in ONE launch.
//
// Reference: /root/reference/stemseg/modeling/backbone/resnet.py:262-282 (Bottleneck.forward: conv1 -> conv2 -> conv3 -> += identity ->
// relu), two consecutive blocks of a stage (:105-113).  As two launches of conv_igemm.h the 4 MID-channel block output is written by
// conv3 and read again by the next conv1 (and later by the next conv3 as its identity): at layer 3 (MID = 256, 32 frames) 212 MB of the
// 742 MB the pair moves.  Here a workgroup owns 256 positions and walks ALL 4 MID output channels of conv3 in co-tiles of CT: the co-tile's
// accumulators get scale / bias / identity / ReLU in registers, are written to HBM once (the next block's identity needs them) and -- split
// into the fp16 (hi, lo * 2^11) pairs -- ARE the B operand of conv1's next K-chunk: the MFMA C/D layout gives a lane 16 of a 32-channel
// tile's rows for its own position, a v_permlane32_swap between the lane halves turns them into the two 16-deep k-groups in the standalone
// kernel's k order.  conv1's MID x 256 accumulators stay in registers through the whole launch.
//
// Same operands, same split arithmetic (split_pair_f16), same k order per accumulator as conv_igemm_kernel's 1x1 tiles (32-channel chunks, two
// k-groups of one tap x 16 channels, products lo_w*hi_x, (hi_w 2^-11)*(lo_x 2^11), hi_w*hi_x) => BIT-IDENTICAL to the two launches whenever
// those run without split-K (tests/test_gpu_fused_tail.py).
//
// Data movement: everything staged by LDS-DMA (global_load_lds_dwordx4, no staging registers, no VALU):
//   * conv3's input -- conv2's output -- arrives ALREADY SPLIT: conv2's epilogue writes the fp16 pair planes ("P16", conv_igemm.h) instead
//     of fp32, same 4 bytes per value, in octets: word [plane][channel / 8][position][(channel % 8) / 2] -- a lane's eight k-values of a
//     k-group are ONE ds_read_b128;
//   * weights in the packed f16x3 layout of stemseg_hip_pack_conv_weight_prec, unchanged: conv3's [chunk][grp][plane][half][4 MID][16 B]
//     has the co-tile's CT channels as one 16 CT-byte run per row, conv1's chunks [..][MID][16 B] for a co-tile are one contiguous block.
// Stages: per co-tile MID / 32 conv3 sub-stages (x chunk + w3 chunk double-buffered, a share of the co-tile's w1 block streamed in beside
// them), then ONE epilogue + conv1 stage.  One barrier per stage, vmcnt(0) in front of it.
//
// Shortcut variants (DS > 0; the first block of stages 1-2, resnet.py:262-282 with a downsample branch): the block's projection shortcut
// (1x1, DS -> 4 MID, + bias) is summed HERE, per co-tile in front of conv3's stages -- its packed weights through the same w3 buffers and
// stage machinery, the block's fp32 input loaded by the wave and split in registers with split_pair_f16, an accumulator of its own, then
// x 1 / scale and + bias as two rounded steps -- and stands where the loaded identity rows stand otherwise.  Same operands, products and k
// order as the stand-alone <1,1,1,32,...> launch => the same bits (tests/test_gpu_fused_shortcut.py); the shortcut map is never written.
//
// Stage-end variants (LAT; the last block of stages 1-3, resnet.py:262-282 and fpn.py:47-69 of the reference): the conv1 slot -- N1 output channels,
// separate from MID -- takes the stage's FPN lateral (1x1, 4 MID -> 256: fpn_inner_w / fpn_inner_b, packed with conv1's geometry) instead of the next
// block's conv1: the stage output is written once, the same values split in registers feed the lateral's K loop, and its epilogue -- x 1 / scale, + bias
// as two rounded steps, NO ReLU -- writes the dense [256][V] map the FPN's add pass reads.  The lanes whose position has even (y, x) also store their
// value into p.xsub: out[c][t][y / 2][x / 2], what subsample2_kernel makes for the next stage's first block (buffer stores with a loop-invariant lane
// offset; every other lane carries an offset the descriptor's range check drops).  The lateral is the same GEMM the stand-alone 256-channel tile runs
// un-split: 32-channel chunks ascending from a zero accumulator => the same bits (tests/test_gpu_stage_end_tail.py); the stage output is not read back
// by the lateral, and the sub-sample pass is gone.  Stages 2-3: the one-wave-per-SIMD form (MID = 128: N1 = 256 are eight slot steps like MID = 256's);
// stage 1: the 32-column form with a 64-channel co-tile (MID = 64 is ONE conv3 stage of the one-wave form, which needs two).
#include "common.h"
#include "split_operand.h"

namespace stemseg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct FusedTailParams {
    const unsigned int* x16;     // conv2's output as fp16 pair planes: [2][MID / 8][V][4] words
    const char* w3;              // packed f16x3 weights of conv3 (Cout = 4 MID, Cin = MID, 1 tap) + float inv[4 MID] behind the slabs
    const float* b3;
    const float* res;            // identity: dense [4 MID][V]
    float* y;                    // block output: dense [4 MID][V]
    const char* w1;              // packed f16x3 weights of the next block's conv1 (Cout = MID, Cin = 4 MID) + float inv[MID]
    const float* b1;
    float* z;                    // conv1 output (+ bias, ReLU) at (t, y, x) of a [MID][T][h + 2][pitch] zero-haloed interior view
    int64_t z_cs, z_ts, z_ys;
    int dec_H, dec_W;
    int V;                       // positions: T * h * w
    // shortcut variants (DS > 0) only: the block's projection shortcut (1x1, DS -> 4 MID, + bias) is computed here and takes the place of `res`
    const float* xs;             // its input, the block's input map: dense [DS][V]
    const char* wd;              // its packed f16x3 weights (Cout = 4 MID, Cin = DS) + float inv[4 MID] behind the slabs
    const float* bd;
    // stage-end variants (LAT) only: the kept quarter of the block output, out[c][t][y / 2][x / 2] = y[c][t][y][x] at even (y, x) -- the input of
    // the next stage's first block (encoder.hip, subsample2_kernel)
    float* xsub;                 // dense [4 MID][sub_V]
    int sub_V;                   // T * (dec_H / 2) * (dec_W / 2)
};

// the packed f16x3 layout of a 1x1 convolution (split_operand.h): 32-channel chunks of two k-groups x (hi, lo) x two lane halves; the tile
// configurations below keep byte sizes of their own and tie them to it
constexpr SplitLayout FT_WL = SplitLayout(1, STEMSEG_PRECISION_F16X3);
static_assert(FT_WL.CK == 32 && FT_WL.G == 2 && FT_WL.NPL == 2, "the fused tail walks 32-channel chunks of two k-groups, two planes");

// what the conv1 slot's epilogue does with a finished value: conv1 of the next block ends in a ReLU, the FPN lateral of a stage-end variant does not
template <bool LAT>
__device__ __forceinline__ float slot_act(const float v) { return LAT ? v : relu_keep_nan(v); }

template <int MID_, int CT_, int P_, int DS_ = 0, int N1_ = MID_, bool LAT_ = false>
struct FusedTailCfg {
    static constexpr int MID = MID_, CT = CT_, COUT = 4 * MID_;
    static constexpr int N1 = N1_;                          // output channels of the conv1 slot: the next block's conv1 (MID), or the stage's FPN lateral (256)
    static constexpr bool LAT = LAT_;                       // stage-end variant: the slot is the FPN lateral (no ReLU, dense map), and the kept quarter of y goes to p.xsub
    static constexpr int DS = DS_, NCD = DS_ / 32;          // shortcut variant: its input channels / K-chunks (0: the identity comes from p.res)
    static constexpr int P = P_, NW = P_ / 32, NTHREADS = 64 * NW;   // positions per workgroup; one 32-position column block per wave
    static constexpr int NC3 = MID / 32;                   // conv3 K-chunks (32 channels)
    static constexpr int NCT = COUT / CT;                  // co-tiles
    static constexpr int MI3 = CT / 32, MI1 = N1 / 32;     // 32-row accumulator tiles per wave: conv3 co-tile, conv1 slot
    static constexpr int NH = 2 * MI3;                     // conv1 K-halves (k-groups of 16 channels) per co-tile
    static constexpr int UNROLL3 = LAT && NC3 <= 2 ? NC3 : 1;  // conv3's chunk loop: rolled -- but MID = 64's two chunks unrolled beside the lateral's 128 accumulator registers (rolled, that loop spills a tile of them)
    static constexpr int X_BYTES = 2 * 4 * P * 16;          // x chunk: [plane][octet][position][4 words]
    static constexpr int W3_BYTES = 8 * CT * 16;            // w3 chunk of the co-tile: [grp][plane][half][CT][16 B]
    static constexpr int W1_HALF = 4 * N1 * 16;             // one k-group of w1: [plane][half][N1][16 B]; a co-tile's NH of them are contiguous in the packed blob
    static constexpr int LDS_BYTES = 2 * X_BYTES + 2 * W3_BYTES + 2 * W1_HALF;
    static constexpr int NQ = P / 64;                       // 64-position quarters of an x row
    static constexpr int X_PIECES = X_BYTES / 1024, W3_PIECES = W3_BYTES / 1024, W1_PIECES = W1_HALF / 1024;     // 1 KB wave-instructions
    static_assert(NC3 == FT_WL.chunks(MID) && W3_BYTES == FT_WL.slab_bytes(CT, 32) && W1_HALF * FT_WL.G == FT_WL.slab_bytes(N1, 32), "tile byte sizes follow the packed-weight layout");
    static_assert(P % 64 == 0 && MID % 32 == 0 && N1 % 32 == 0 && CT % 32 == 0 && COUT % CT == 0 && 2 * N1 * 4 <= 2 * X_BYTES, "tile shapes");
    static_assert(LDS_BYTES <= (P <= 128 ? 80 : 160) * 1024, "LDS: two 128-position workgroups, or one 256-position workgroup, per CU");
    static_assert(W3_BYTES % 1024 == 0 && W1_HALF % 1024 == 0 && X_PIECES % NW == 0, "whole DMA pieces");
    static_assert(MI1 * 16 + MI3 * 16 + (DS ? MI3 * 16 : 0) <= 176, "accumulators must leave room for fragments at 256 registers");
    static_assert(DS % 32 == 0 && 2 * CT * 4 <= W1_HALF, "shortcut: whole K-chunks; its (1 / scale, bias) table waits in a w1 buffer");
};

// Stages of a workgroup, one barrier (behind a vmcnt(0)) each; every stage first requests what the NEXT stage reads (LDS-DMA into the idle
// buffer of its kind), then computes:
//   per co-tile j:  S(c), c < MID / 32   conv3 MFMAs of K-chunk c (x chunk c + w3 chunk (j, c)); the last one also requests w1 half 0 and the
//                                        identity values of the co-tile's first 32-channel tile
//                   E(h), h < 2 CT / 32  h even: scale / bias / identity / ReLU / store / split of 32-channel tile h / 2, its two k-groups as B
//                                        fragments; then conv1's MFMAs of k-group h (w1 half h); the last one requests the next co-tile's S(0)
// A stage is 0.4-0.8 us of matrix work against ~1 us from a DMA request to its landing, so one workgroup alone spends most of its time at the
// barrier (measured: the 256-position form ran at 34 % MFMA-pipe occupancy, and removing ALL its MFMAs saved 9 %).  The 128-position form is
// therefore the default: 80 KB of LDS, four waves -- TWO workgroups per CU, each filling the other's waits.
template <class C>
__global__ __launch_bounds__(C::NTHREADS, 2) void fused_tail_kernel(const FusedTailParams p) {
#pragma clang fp contract(off)       // scale, bias and identity are separately rounded steps in the standalone kernels: no multiply-add contraction here
    __shared__ __attribute__((aligned(1024))) char smem[C::LDS_BYTES];
    char* const xbuf = smem;                               // 2 buffers
    char* const w3buf = smem + 2 * C::X_BYTES;             // 2 buffers
    char* const w1buf = smem + 2 * C::X_BYTES + 2 * C::W3_BYTES;      // 2 buffers (k-group halves)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int pos0 = blockIdx.x * C::P;
    const int pos = pos0 + wave * 32 + l31;                // this lane's position (column of every accumulator tile of the wave)
    const bool pos_ok = pos < p.V;
    const int pos_c = min(pos, p.V - 1);                    // (loads of a column past V read the last valid one: the column is never stored)
    const int64_t V = p.V;
    // Addressing: every global access below is (wave-uniform 64-bit base in SGPRs) + (ONE loop-invariant 32-bit per-lane byte offset), so that
    // no 64-bit per-lane pointer stays live across the stages (the first build kept ~50 of them and spilled them around every DMA issue).
    // The channel of accumulator register r of lane half h is base + (r & 3) + 8 (r >> 2) + 4 h: the 4 h part goes into the lane offset.
    const unsigned int lane_off = (unsigned int)(((int64_t)(4 * half) * V + pos_c) * 4);      // bytes: (4 half) channels down, this lane's column
    auto opaque = [](unsigned int v) __attribute__((always_inline)) { asm volatile("" : "+v"(v)); return v; };   // (keeps address arithmetic inside its stage)
    // stage-end variant: this lane's column of the kept quarter -- its position is (t, y, x) of [T][dec_H][dec_W] planes, kept where y and x are even
    // (buffer stores: the channel row is an SGPR offset, and every other lane carries an offset the descriptor's range check drops)
    const unsigned int SV4 = C::LAT ? (unsigned int)p.sub_V * 4u : 0u;
    unsigned int sub_off = 0xFFFFFF00u;
    if constexpr (C::LAT) {
        const int hwp = p.dec_H * p.dec_W, t2 = pos_c / hwp, r2 = pos_c - t2 * hwp, y2 = r2 / p.dec_W, x2 = r2 - y2 * p.dec_W;
        if (pos_ok && !((y2 | x2) & 1)) sub_off = (unsigned int)(4 * half) * SV4 + (unsigned int)((t2 * (p.dec_H / 2) + y2 / 2) * (p.dec_W / 2) + x2 / 2) * 4u;
    }

    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const float* inv3 = reinterpret_cast<const float*>(p.w3 + FT_WL.inv_offset(C::COUT, C::MID));
    const float* inv1 = reinterpret_cast<const float*>(p.w1 + FT_WL.inv_offset(C::N1, C::COUT));

    // ---- DMA issue helpers (each call = this wave's share; 1 KB per wave instruction, LDS image lane-linear) -------------------------
    const int xpos = min(pos0 + lane, p.V - 1);             // (clamped: columns past V are computed and never stored)
    auto dma_x = [&](const int c, const int buf) __attribute__((always_inline)) {       // x chunk c: (plane, octet, 64-position quarter) pieces
#pragma unroll
        for (int k = 0; k < C::X_PIECES / C::NW; ++k) {
            const int idx = wave * (C::X_PIECES / C::NW) + k, q = idx % C::NQ, o = (idx / C::NQ) & 3, pl = idx / (4 * C::NQ);
            const unsigned int xp = (unsigned int)min((int)opaque((unsigned int)xpos) + q * 64, p.V - 1);
            const char* src = reinterpret_cast<const char*>(p.x16) + ((int64_t)(pl * (C::MID / 8) + 4 * c + o)) * V * 16 + (size_t)(xp * 16u);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(xbuf + buf * C::X_BYTES + ((pl * 4 + o) * C::P + q * 64) * 16), 16, 0, 0);
        }
    };
    // chunk (co-tile j, K-chunk c) of a packed [..][4 MID][16 B] blob -- conv3's or the shortcut's: 8 rows of CT x 16 B
    auto dma_wc = [&](const char* blob, const int j, const int c, const int buf) __attribute__((always_inline)) {
        constexpr int PER_ROW = C::CT * 16 / 1024;
#pragma unroll
        for (int k = 0; k < (C::W3_PIECES + C::NW - 1) / C::NW; ++k) {
            const int idx = wave + k * C::NW;
            if (idx < C::W3_PIECES) {
                const int row = idx / PER_ROW, part = idx % PER_ROW;
                const char* src = blob + ((int64_t)c * 8 + row) * (C::COUT * 16) + (int64_t)j * (C::CT * 16) + part * 1024 + (size_t)(opaque((unsigned int)lane) * 16u);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(w3buf + buf * C::W3_BYTES + idx * 1024), 16, 0, 0);
            }
        }
    };
    auto dma_w3 = [&](const int j, const int c, const int buf) __attribute__((always_inline)) { dma_wc(p.w3, j, c, buf); };
    auto dma_wd = [&](const int j, const int c, const int buf) __attribute__((always_inline)) { dma_wc(p.wd, j, c, buf); };
    auto dma_w1 = [&](const int j, const int h, const int buf) __attribute__((always_inline)) {      // k-group half h of co-tile j's w1 block
#pragma unroll
        for (int k = 0; k < (C::W1_PIECES + C::NW - 1) / C::NW; ++k) {
            const int idx = wave + k * C::NW;
            if (idx < C::W1_PIECES) {
                const char* src = p.w1 + ((int64_t)j * C::NH + h) * C::W1_HALF + (int64_t)idx * 1024 + (size_t)(opaque((unsigned int)lane) * 16u);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(w1buf + buf * C::W1_HALF + idx * 1024), 16, 0, 0);
            }
        }
    };
    // the co-tile's per-channel (1 / scale, bias): CT + CT floats into the head of the w3 buffer that idles through the epilogue stages
    // (lanes 0 .. CT / 4 - 1 of wave 0 carry the scales, the next CT / 4 lanes the biases)
    auto dma_tab = [&](const int j, const int buf) __attribute__((always_inline)) {
        static_assert(2 * (C::CT / 4) <= 64 && 2 * C::CT * 4 <= C::W3_BYTES, "the table is one DMA piece");
        if (wave == 0 && lane < 2 * (C::CT / 4)) {
            const unsigned int l = opaque((unsigned int)lane);
            const float* src = (l < C::CT / 4 ? inv3 : p.b3 - C::CT) + (int64_t)j * C::CT + (size_t)(l * 4u);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(w3buf + buf * C::W3_BYTES), 16, 0, 0);
        }
    };
    // shortcut variant: the same table of the shortcut's co-tile, into w1 buffer 1 -- idle from the barrier behind the previous co-tile's last
    // k-group until this co-tile's first epilogue stage requests k-group 1; the table is consumed right behind the shortcut's last stage
    auto dma_dtab = [&](const int j) __attribute__((always_inline)) {
        if (wave == 0 && lane < 2 * (C::CT / 4)) {
            const unsigned int l = opaque((unsigned int)lane);
            const float* invd = reinterpret_cast<const float*>(p.wd + FT_WL.inv_offset(C::COUT, C::DS));
            const float* src = (l < C::CT / 4 ? invd : p.bd - C::CT) + (int64_t)j * C::CT + (size_t)(l * 4u);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(w1buf + C::W1_HALF), 16, 0, 0);
        }
    };
    // shortcut variant: the wave's share of the shortcut's input, fp32 -- k-group G (16 channels), lane (half, n): channels 16 G + 8 half + 0 .. 7 at
    // its position, the packed weights' k order.  The same values for every co-tile: requested a stage ahead of each, split at its top.
    // (buffer loads: the channel row is an SGPR offset, the lane offset loop-invariant -- per-lane 64-bit addresses would stay live across the stages)
    constexpr int NXS = C::DS > 0 ? C::DS / 2 : 1;
    auto load_xs = [&](float (&xr)[NXS]) __attribute__((always_inline)) {
        const unsigned int V4 = (unsigned int)p.V * 4u;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.xs), 0, (int)((unsigned int)C::DS * V4), 0x00020000);
        const unsigned int off = (unsigned int)(8 * half) * V4 + (unsigned int)pos_c * 4u;
#pragma unroll
        for (int i = 0; i < C::DS / 2; ++i)
            xr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, (unsigned int)(16 * (i >> 3) + (i & 7)) * V4, 0));
    };
    // the conv1 slot's own (1 / scale, bias): N1 + N1 floats into the (by then idle) x buffer, requested in the very last stage
    auto dma_tail_tab = [&]() __attribute__((always_inline)) {
        constexpr int PIECES = (2 * C::N1 + 255) / 256;
        static_assert(PIECES <= C::NW, "one piece per wave");
        if (wave < PIECES) {
            const unsigned int f0 = (unsigned int)wave * 256u + opaque((unsigned int)lane) * 4u;
            if (f0 < 2u * C::N1) {
                const float* src = (f0 < (unsigned int)C::N1 ? inv1 : p.b1 - C::N1) + (size_t)f0;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(xbuf + wave * 1024), 16, 0, 0);
            }
        }
    };
    auto stage_sync = [&]() __attribute__((always_inline)) {
        // vmcnt(0): this wave's DMA pieces (and loads / stores) have landed.  The BUILTIN, not inline assembly: the compiler's wait-count
        // pass must see it, or it guards the first use of a value loaded a stage earlier with a vmcnt(0) of its own -- behind the DMA
        // just issued for the next stage
        __builtin_amdgcn_s_waitcnt(0x0f70);
        __syncthreads();
    };
    auto load_identity = [&](const int co_first, float (&rres)[16]) __attribute__((always_inline)) {   // rows of the 32-channel tile at co_first, this lane's column
#pragma unroll
        for (int r = 0; r < 16; ++r)
            rres[r] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.res + (int64_t)(co_first + (r & 3) + 8 * (r >> 2)) * V) + (size_t)lane_off);
    };

    f32x16 acc1[C::MI1];
#pragma unroll
    for (int m = 0; m < C::MI1; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[m][r] = 0.f;

    const f16x8 k2048 = {(_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE),
                         (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE)};

    // three products per (A, B) fragment pair, smallest first -- the order of conv_igemm.h's f16x3 stream
    auto mma3 = [&](f32x16& acc, const f16x8 a_hi, const f16x8 a_lo, const f16x8 b_hi, const f16x8 b_lo) __attribute__((always_inline)) {
        const f16x8 a_his = a_hi * k2048;                    // hi_w * 2^-11 (exact: a power of two on a normal number)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_his, b_lo, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc, 0, 0, 0);
    };

    constexpr bool DSV = C::DS > 0;                          // the shortcut variant
    float xr[NXS];
    if constexpr (DSV) { dma_wd(0, 0, 0); load_xs(xr); }
    else { dma_x(0, 0); dma_w3(0, 0, 0); }
    stage_sync();
    int sb = 0;                                              // x / w3 buffer of the conv3 sub-stage about to run
#pragma unroll 1
    for (int j = 0; j < C::NCT; ++j) {
        // ---- shortcut variant: D(c), c < DS / 32 -- the shortcut's MFMAs of K-chunk c (its weights through the w3 buffers, its input split in
        // registers), in front of the co-tile's conv3 stages; the last one requests S(0).  Scale and bias behind them: accd then holds what the
        // stand-alone launch would have written to the shortcut map, in the registers the epilogue reads the identity from.
        f32x16 accd[DSV ? C::MI3 : 1];
        if constexpr (DSV) {
            f16x8 d_hi[2 * C::NCD], d_lo[2 * C::NCD];
#pragma unroll
            for (int G = 0; G < 2 * C::NCD; ++G) {
                u32x4 hw4, lw4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    unsigned int hwd, lwd;
                    split_pair_f16(xr[8 * G + 2 * i], xr[8 * G + 2 * i + 1], hwd, lwd);
                    hw4[i] = hwd; lw4[i] = lwd;
                }
                d_hi[G] = __builtin_bit_cast(f16x8, hw4);
                d_lo[G] = __builtin_bit_cast(f16x8, lw4);
            }
#pragma unroll
            for (int m = 0; m < C::MI3; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) accd[m][r] = 0.f;
#pragma unroll
            for (int c = 0; c < C::NCD; ++c) {
                if (c + 1 < C::NCD) dma_wd(j, c + 1, sb ^ 1);
                else { dma_x(0, sb ^ 1); dma_w3(j, 0, sb ^ 1); }
                if (c == 0) dma_dtab(j);
                const char* wb = w3buf + sb * C::W3_BYTES + (half * C::CT + l31) * 16;
                constexpr int NS = 2 * C::MI3;
                f16x8 a_hi[2], a_lo[2];
                auto ld_a = [&](const int st, const int k) __attribute__((always_inline)) {
                    const int g = st / C::MI3, m = st % C::MI3;
                    a_hi[k] = *reinterpret_cast<const f16x8*>(wb + (((g * 2 + 0) * 2) * C::CT + m * 32) * 16);
                    a_lo[k] = *reinterpret_cast<const f16x8*>(wb + (((g * 2 + 1) * 2) * C::CT + m * 32) * 16);
                };
                ld_a(0, 0);
#pragma unroll
                for (int st = 0; st < NS; ++st) {
                    if (st + 1 < NS) ld_a(st + 1, (st + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
                    mma3(accd[st % C::MI3], a_hi[st & 1], a_lo[st & 1], d_hi[2 * c + st / C::MI3], d_lo[2 * c + st / C::MI3]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                stage_sync();
                sb ^= 1;
            }
            const float* dtab = reinterpret_cast<const float*>(w1buf + C::W1_HALF);
#pragma unroll
            for (int m = 0; m < C::MI3; ++m)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 sc = *reinterpret_cast<const float4*>(dtab + m * 32 + 8 * q + 4 * half);
                    const float4 bv = *reinterpret_cast<const float4*>(dtab + C::CT + m * 32 + 8 * q + 4 * half);
                    accd[m][4 * q + 0] = __fadd_rn(__fmul_rn(accd[m][4 * q + 0], sc.x), bv.x);
                    accd[m][4 * q + 1] = __fadd_rn(__fmul_rn(accd[m][4 * q + 1], sc.y), bv.y);
                    accd[m][4 * q + 2] = __fadd_rn(__fmul_rn(accd[m][4 * q + 2], sc.z), bv.z);
                    accd[m][4 * q + 3] = __fadd_rn(__fmul_rn(accd[m][4 * q + 3], sc.w), bv.w);
                }
            // (pinned here: sunk to the epilogues that read them, these sums would leave the whole table live in registers across the conv3 stages)
#pragma unroll
            for (int m = 0; m < C::MI3; ++m) asm volatile("" : "+v"(accd[m]));
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x16 acc3[C::MI3];
#pragma unroll
        for (int m = 0; m < C::MI3; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc3[m][r] = 0.f;
        const int co_j = j * C::CT;
        float rres[16];                                      // identity values of the 32-channel tile whose epilogue comes next
#pragma unroll C::UNROLL3
        for (int c = 0; c < C::NC3; ++c) {
            if (c + 1 < C::NC3) { dma_x(c + 1, sb ^ 1); dma_w3(j, c + 1, sb ^ 1); }
            else { dma_w1(j, 0, 0); dma_tab(j, sb ^ 1); if constexpr (!DSV) load_identity(co_j, rres); }
            const char* xb = xbuf + sb * C::X_BYTES + (half * C::P + wave * 32 + l31) * 16;
            const char* wb = w3buf + sb * C::W3_BYTES + (half * C::CT + l31) * 16;
            // software pipeline over the (k-group, 32-row tile) steps: the A fragments of step s + 1 are requested before the MFMAs of step s
            // issue; fenced, or the scheduler hoists every fragment of the stage to its top (and spills) or sinks each to its use
            constexpr int NS = 2 * C::MI3;
            f16x8 b_hi[2], b_lo[2], a_hi[2], a_lo[2];
            auto ld_b = [&](const int g, const int k) __attribute__((always_inline)) {
                b_hi[k] = *reinterpret_cast<const f16x8*>(xb + ((0 * 4 + 2 * g) * C::P) * 16);
                b_lo[k] = *reinterpret_cast<const f16x8*>(xb + ((1 * 4 + 2 * g) * C::P) * 16);
            };
            auto ld_a = [&](const int st, const int k) __attribute__((always_inline)) {
                const int g = st / C::MI3, m = st % C::MI3;
                a_hi[k] = *reinterpret_cast<const f16x8*>(wb + (((g * 2 + 0) * 2) * C::CT + m * 32) * 16);
                a_lo[k] = *reinterpret_cast<const f16x8*>(wb + (((g * 2 + 1) * 2) * C::CT + m * 32) * 16);
            };
            ld_b(0, 0);
            ld_b(1, 1);
            ld_a(0, 0);
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                if (st + 1 < NS) ld_a(st + 1, (st + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
                mma3(acc3[st % C::MI3], a_hi[st & 1], a_lo[st & 1], b_hi[st / C::MI3], b_lo[st / C::MI3]);
                __builtin_amdgcn_sched_barrier(0);
            }
            stage_sync();
            sb ^= 1;
        }
        // ---- epilogue of the co-tile + its K-halves of conv1 ---------------------------------------------------------------------------
        f16x8 b_hi[2], b_lo[2];                              // the two k-groups of the current 32-channel tile as B fragments
#pragma unroll
        for (int h = 0; h < C::NH; ++h) {
            const int m = h >> 1, g = h & 1;
            if (g == 0) {
                const int co_m = co_j + m * 32;
                // scale back, + bias, + identity, ReLU, store; C/D layout: register r of lane (half, l31) = row (r & 3) + 8 (r >> 2) + 4 half
                unsigned int hw[8], lw[8];
                const float* tab = reinterpret_cast<const float*>(w3buf + sb * C::W3_BYTES);      // (dma_tab: requested in the last conv3 sub-stage)
                if constexpr (DSV) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) rres[r] = accd[m][r];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co4 = co_m + 8 * q + 4 * half;
                    const float4 sc = *reinterpret_cast<const float4*>(tab + (co4 - co_j));
                    const float4 bv = *reinterpret_cast<const float4*>(tab + C::CT + (co4 - co_j));
                    // (explicitly rounded steps: the standalone kernel scales its accumulators in one place and adds bias / identity in another)
                    float v0 = __fmul_rn(acc3[m][4 * q + 0], sc.x), v1 = __fmul_rn(acc3[m][4 * q + 1], sc.y), v2 = __fmul_rn(acc3[m][4 * q + 2], sc.z),
                          v3 = __fmul_rn(acc3[m][4 * q + 3], sc.w);
                    v0 = relu_keep_nan(__fadd_rn(__fadd_rn(v0, bv.x), rres[4 * q + 0]));
                    v1 = relu_keep_nan(__fadd_rn(__fadd_rn(v1, bv.y), rres[4 * q + 1]));
                    v2 = relu_keep_nan(__fadd_rn(__fadd_rn(v2, bv.z), rres[4 * q + 2]));
                    v3 = relu_keep_nan(__fadd_rn(__fadd_rn(v3, bv.w), rres[4 * q + 3]));
                    if (pos_ok) {
                        char* yo = reinterpret_cast<char*>(p.y + (int64_t)(co_m + 8 * q) * V);       // (uniform; the 4 half rows are in lane_off)
                        *reinterpret_cast<float*>(yo + (size_t)lane_off) = v0;
                        *reinterpret_cast<float*>(yo + V * 4 + (size_t)lane_off) = v1;
                        *reinterpret_cast<float*>(yo + V * 8 + (size_t)lane_off) = v2;
                        *reinterpret_cast<float*>(yo + V * 12 + (size_t)lane_off) = v3;
                    }
                    if constexpr (C::LAT) {
                        const __amdgpu_buffer_rsrc_t rsub = __builtin_amdgcn_make_buffer_rsrc(p.xsub + (int64_t)co_j * p.sub_V, 0, (int)((unsigned int)C::CT * SV4), 0x00020000);
                        const unsigned int row = (unsigned int)(m * 32 + 8 * q);                          // (within the co-tile; the 4 half rows are in sub_off)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v0), rsub, sub_off, (row + 0) * SV4, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v1), rsub, sub_off, (row + 1) * SV4, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v2), rsub, sub_off, (row + 2) * SV4, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v3), rsub, sub_off, (row + 3) * SV4, 0);
                    }
                    split_pair_f16(v0, v1, hw[2 * q], lw[2 * q]);
                    split_pair_f16(v2, v3, hw[2 * q + 1], lw[2 * q + 1]);
                }
                __builtin_amdgcn_sched_barrier(0);
                // k-groups of 16 channels in the standalone kernel's order: lane half 0 channels 0..7, half 1 channels 8..15 of the group.  The
                // lane halves hold (q even: ch 0-3 | 4-7), (q odd: 8-11 | 12-15): swapping the upper half of the q-even words with the lower half
                // of the q-odd words gives (0-3, 4-7) to half 0 and (8-11, 12-15) to half 1.
#pragma unroll
                for (int gg = 0; gg < 2; ++gg) {
                    unsigned int xh[2], yh[2], xl[2], yl[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        auto sh = __builtin_amdgcn_permlane32_swap(hw[4 * gg + i], hw[4 * gg + 2 + i], false, false);
                        xh[i] = sh[0]; yh[i] = sh[1];
                        auto sl = __builtin_amdgcn_permlane32_swap(lw[4 * gg + i], lw[4 * gg + 2 + i], false, false);
                        xl[i] = sl[0]; yl[i] = sl[1];
                    }
                    const u32x4 bh = {xh[0], xh[1], yh[0], yh[1]}, bl = {xl[0], xl[1], yl[0], yl[1]};
                    b_hi[gg] = __builtin_bit_cast(f16x8, bh);
                    b_lo[gg] = __builtin_bit_cast(f16x8, bl);
                }
            } else if (m + 1 < C::MI3) {
                if constexpr (!DSV) load_identity(co_j + (m + 1) * 32, rres);        // (they land under this k-group's MFMAs)
            }
            __builtin_amdgcn_sched_barrier(0);
            // what the next stage reads (requested behind the epilogue: its table reads are LDS reads the compiler cannot tell from the DMA's target)
            if (h + 1 < C::NH) dma_w1(j, h + 1, (h + 1) & 1);
            else if (j + 1 < C::NCT) {
                if constexpr (DSV) { dma_wd(j + 1, 0, sb); load_xs(xr); }
                else { dma_x(0, sb); dma_w3(j + 1, 0, sb); }
            } else dma_tail_tab();
            const char* w1b = w1buf + (h & 1) * C::W1_HALF + (half * C::N1 + l31) * 16;
            f16x8 a_hi[2], a_lo[2];
            auto ld_a1 = [&](const int m1, const int k) __attribute__((always_inline)) {
                a_hi[k] = *reinterpret_cast<const f16x8*>(w1b + ((0 * 2) * C::N1 + m1 * 32) * 16);
                a_lo[k] = *reinterpret_cast<const f16x8*>(w1b + ((1 * 2) * C::N1 + m1 * 32) * 16);
            };
            ld_a1(0, 0);
#pragma unroll
            for (int m1 = 0; m1 < C::MI1; ++m1) {
                if (m1 + 1 < C::MI1) ld_a1(m1 + 1, (m1 + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
                mma3(acc1[m1], a_hi[m1 & 1], a_lo[m1 & 1], b_hi[g], b_lo[g]);
                __builtin_amdgcn_sched_barrier(0);
            }
            stage_sync();
        }
    }
    // ---- conv1's epilogue: scale back, + bias, ReLU, flat position -> (t, y, x) of the zero-haloed consumer layout -------------------------
    if (pos_ok) {
        const int hwp = p.dec_H * p.dec_W;
        const int t2 = pos / hwp, r2 = pos - t2 * hwp, y2 = r2 / p.dec_W, x2 = r2 - y2 * p.dec_W;
        const unsigned int z_off = (unsigned int)(((int64_t)(4 * half) * p.z_cs + (int64_t)t2 * p.z_ts + (int64_t)y2 * p.z_ys + x2) * 4);      // bytes
#pragma unroll
        for (int m1 = 0; m1 < C::MI1; ++m1)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co4 = m1 * 32 + 8 * q + 4 * half;
                const float4 sc = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(xbuf) + co4);
                const float4 bv = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(xbuf) + C::N1 + co4);
                char* zo = reinterpret_cast<char*>(p.z + (int64_t)(m1 * 32 + 8 * q) * p.z_cs);     // (uniform)
                *reinterpret_cast<float*>(zo + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 0], sc.x), bv.x));
                *reinterpret_cast<float*>(zo + p.z_cs * 4 + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 1], sc.y), bv.y));
                *reinterpret_cast<float*>(zo + p.z_cs * 8 + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 2], sc.z), bv.z));
                *reinterpret_cast<float*>(zo + p.z_cs * 12 + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 3], sc.w), bv.w));
            }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// The 16-column form (MID = 256: layer 3, 22 of the 27 fused launches of an R-101 pass).  What bounds the 32-column form there is not its
// matrix work but its memory-side traffic (profiles/r06e_pmc_fused_tail_256_p128.txt: FETCH + WRITE 1.5 GB per launch against 0.53 GB of
// tensors): conv3's input tile -- 1 KB per position -- is re-read once per co-tile, 16 times, and with every position of the map in flight
// at once those re-reads can only come from the Infinity Cache.  It cannot stay in LDS next to the weight streams (128 KB for 128 positions),
// and as B fragments of 32 positions it is 128 registers beside 160 of accumulators.  With v_mfma_f32_16x16x32_f16 a wave owns 16 positions:
// conv1's accumulators are 64 registers, a 128-channel co-tile's 32, and the wave's WHOLE conv3 input -- 256 channels x 16 positions as
// fp16 pairs -- is 64 registers, loaded once.  LDS then holds weights only (two conv3 chunks and one conv1 k-step per stage, double
// buffered: 128 KB), a stage is 48 MFMAs per wave, and the kernel's traffic is its tensors'.
//   * one MFMA consumes a whole 32-channel chunk (k = 32): lane (n, kb) carries channels 8 kb .. 8 kb + 7 of the chunk -- for conv3 exactly the
//     packed weights' (k-group kb / 2, half kb % 2) vector and the producer's octet 4 s + kb;
//   * C/D layout: lane (n, rb) holds rows 4 rb .. 4 rb + 3 of a 16-row tile.  Two consecutive tiles (32 channels) of the finished co-tile become
//     conv1's next B fragment -- lane (n, kb): channels 8 kb .. 8 kb + 7, the packed w1's own order -- by one v_permlane32_swap and one
//     v_permlane16_swap per word.  (Leaving the rows where they are and fetching the matching A fragment as two 8-byte halves was measured first:
//     the compiler fuses the halves into ds_read2_b64, whose 16-lane groups hit 32 banks at a 16-byte stride -- 39 % of the LDS cycles were
//     bank conflicts, profiles/r06f_pmc_fused_tail16_first.txt.)
// The summation order inside an MFMA differs from the 32x32x16 kernels' (32 channels per instruction instead of two groups of 16), so this
// form agrees with the separate launches to fp32 round-off, not bit for bit; like every kernel here it has ONE summation order whatever the
// batch (no split-K, no dependence on the launch shape).
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int MID_>
struct FusedTail16Cfg {
    static constexpr int MID = MID_, COUT = 4 * MID_, CT = 128;
    static constexpr int NW = 8, NTHREADS = 512, P = 16 * NW;
    static constexpr int NC3 = MID / 32, NCT = COUT / CT;
    static constexpr int NT3 = CT / 16, NT1 = MID / 16;     // 16-row accumulator tiles: conv3 co-tile, conv1
    static constexpr int SC = 2;                            // conv3 chunks per stage
    static constexpr int NS = NC3 / SC, NU = CT / 32;       // conv3 stages / conv1 k-steps per co-tile
    static constexpr int W3_CHUNK = 8 * CT * 16;            // [grp][plane][half][CT][16 B]
    static constexpr int W3_BYTES = SC * W3_CHUNK;
    static constexpr int W1_BYTES = 8 * MID * 16;           // one 32-channel k-step of conv1: [grp][plane][half][MID][16 B]
    static constexpr int TAB_BYTES = 2 * CT * 4;
    static constexpr int LDS_BYTES = 2 * W3_BYTES + 2 * W1_BYTES + 2 * TAB_BYTES;
    static_assert(NC3 % SC == 0 && W3_BYTES % (1024 * NW) == 0 && W1_BYTES % (1024 * NW) == 0 && TAB_BYTES == 1024, "whole DMA pieces per wave");
    static_assert(W3_CHUNK == FT_WL.slab_bytes(CT, FT_WL.CK) && W1_BYTES == FT_WL.slab_bytes(MID, FT_WL.CK), "tile byte sizes follow the packed-weight layout");
    static_assert(LDS_BYTES <= 160 * 1024 && 2 * MID * 4 <= W3_BYTES, "LDS");
};

template <class C>
__global__ __launch_bounds__(C::NTHREADS, 2) void fused_tail16_kernel(const FusedTailParams p) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(1024))) char smem[C::LDS_BYTES];
    char* const w3buf = smem;
    char* const w1buf = smem + 2 * C::W3_BYTES;
    char* const tabbuf = smem + 2 * C::W3_BYTES + 2 * C::W1_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kb = lane >> 4;                 // column (position) of the wave's 16 / k-block (inputs) = row-block (accumulators)
    const int pos = blockIdx.x * C::P + wave * 16 + n;
    const bool pos_ok = pos < p.V;
    const int pos_c = min(pos, p.V - 1);
    const int64_t V = p.V;
    const unsigned int lane_off = (unsigned int)(((int64_t)(4 * kb) * V + pos_c) * 4);       // bytes: rows 4 kb .. of a tile, this lane's column
    auto opaque = [](unsigned int v) __attribute__((always_inline)) { asm volatile("" : "+v"(v)); return v; };
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const float* inv3 = reinterpret_cast<const float*>(p.w3 + FT_WL.inv_offset(C::COUT, C::MID));
    const float* inv1 = reinterpret_cast<const float*>(p.w1 + FT_WL.inv_offset(C::MID, C::COUT));

    auto dma_w3 = [&](const int j, const int st, const int buf) __attribute__((always_inline)) {      // chunks SC st .. of co-tile j
        constexpr int PER_ROW = C::CT * 16 / 1024, PER_CHUNK = C::W3_CHUNK / 1024;
#pragma unroll
        for (int k = 0; k < C::W3_BYTES / 1024 / C::NW; ++k) {
            const int idx = wave + k * C::NW, sc = idx / PER_CHUNK, r = idx % PER_CHUNK, row = r / PER_ROW, part = r % PER_ROW;
            const char* src = p.w3 + ((int64_t)(st * C::SC + sc) * 8 + row) * (C::COUT * 16) + (int64_t)j * (C::CT * 16) + part * 1024 + (size_t)(opaque((unsigned int)lane) * 16u);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(w3buf + buf * C::W3_BYTES + idx * 1024), 16, 0, 0);
        }
    };
    auto dma_w1 = [&](const int cc, const int buf) __attribute__((always_inline)) {                   // conv1 k-step (32-channel chunk) cc
#pragma unroll
        for (int k = 0; k < C::W1_BYTES / 1024 / C::NW; ++k) {
            const int idx = wave + k * C::NW;
            const char* src = p.w1 + (int64_t)cc * C::W1_BYTES + (int64_t)idx * 1024 + (size_t)(opaque((unsigned int)lane) * 16u);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(w1buf + buf * C::W1_BYTES + idx * 1024), 16, 0, 0);
        }
    };
    auto dma_tab = [&](const int j) __attribute__((always_inline)) {        // co-tile j's (1 / scale | bias): lanes 0-31 scales, 32-63 biases
        if (wave == 0) {
            const unsigned int l = opaque((unsigned int)lane);
            const float* src = (l < 32 ? inv3 : p.b3 - C::CT) + (int64_t)j * C::CT + (size_t)(l * 4u);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(tabbuf + (j & 1) * C::TAB_BYTES), 16, 0, 0);
        }
    };
    auto dma_tail_tab = [&]() __attribute__((always_inline)) {            // conv1's own (1 / scale | bias) into the idle w3 buffer
        constexpr int PIECES = (2 * C::MID + 255) / 256;
        if (wave < PIECES) {
            const unsigned int f0 = (unsigned int)wave * 256u + opaque((unsigned int)lane) * 4u;
            if (f0 < 2u * C::MID) {
                const float* src = (f0 < (unsigned int)C::MID ? inv1 : p.b1 - C::MID) + (size_t)f0;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(w3buf + wave * 1024), 16, 0, 0);
            }
        }
    };
    auto stage_sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_s_waitcnt(0x0f70);                  // vmcnt(0), as a builtin: see fused_tail_kernel
        __syncthreads();
    };
    auto load_identity = [&](const int co_first, float (&rres)[8]) __attribute__((always_inline)) {    // two 16-row tiles from co_first: rows 4 kb + r
#pragma unroll
        for (int i = 0; i < 8; ++i)
            rres[i] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.res + (int64_t)(co_first + 16 * (i >> 2) + (i & 3)) * V) + (size_t)lane_off);
    };
    const f16x8 k2048 = {(_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE),
                         (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE)};
    // two 16-row tiles per step, their MFMAs alternating: consecutive MFMAs never wait for each other's accumulator (same products, same order
    // per accumulator as mma3)
    auto mma3x2 = [&](f32x4& c0, f32x4& c1, const f16x8 a0_hi, const f16x8 a0_lo, const f16x8 a1_hi, const f16x8 a1_lo, const f16x8 b_hi, const f16x8 b_lo)
        __attribute__((always_inline)) {
        const f16x8 a0_his = a0_hi * k2048, a1_his = a1_hi * k2048;
        c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0_lo, b_hi, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1_lo, b_hi, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0_his, b_lo, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1_his, b_lo, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0_hi, b_hi, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1_hi, b_hi, c1, 0, 0, 0);
    };

    // the first stage's weights, then the wave's whole conv3 input: chunk s, lane (n, kb) = octet 4 s + kb of both planes at its position
    dma_w3(0, 0, 0);
    f16x8 xh[C::NC3], xl[C::NC3];
    {
        const char* xs = reinterpret_cast<const char*>(p.x16) + (size_t)((unsigned int)pos_c * 16u);
#pragma unroll
        for (int s = 0; s < C::NC3; ++s) {
            xh[s] = *reinterpret_cast<const f16x8*>(xs + ((int64_t)(4 * s + kb)) * V * 16);
            xl[s] = *reinterpret_cast<const f16x8*>(xs + ((int64_t)(C::MID / 8 + 4 * s + kb)) * V * 16);
        }
    }
    f32x4 acc1[C::NT1];
#pragma unroll
    for (int m = 0; m < C::NT1; ++m) acc1[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    stage_sync();
    int sb = 0, eb = 0;                                      // buffers of the conv3 stage / the conv1 k-step about to run
#pragma unroll 1
    for (int j = 0; j < C::NCT; ++j) {
        f32x4 acc3[C::NT3];
#pragma unroll
        for (int t = 0; t < C::NT3; ++t) acc3[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int co_j = j * C::CT;
        float rres[8];
#pragma unroll
        for (int st = 0; st < C::NS; ++st) {
            if (st + 1 < C::NS) dma_w3(j, st + 1, sb ^ 1);
            else { dma_w1(j * C::NU, eb); dma_tab(j); load_identity(co_j, rres); }
            const char* wb = w3buf + sb * C::W3_BYTES + (((kb >> 1) * 2 * 2 + (kb & 1)) * C::CT + n) * 16;       // row (g = kb / 2, plane 0, h = kb % 2), this lane's tile row
            constexpr int NSTEP = C::SC * C::NT3 / 2;            // steps of two tiles
            f16x8 a_hi[2][2], a_lo[2][2];                       // (two sets here: the fragments of step i + 1 are requested before the MFMAs of step i issue)
            auto ld_a = [&](const int i, const int k) __attribute__((always_inline)) {
                const int sc = (2 * i) / C::NT3, t = (2 * i) % C::NT3;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    a_hi[k][e] = *reinterpret_cast<const f16x8*>(wb + sc * C::W3_CHUNK + (0 * 2 * C::CT + (t + e) * 16) * 16);
                    a_lo[k][e] = *reinterpret_cast<const f16x8*>(wb + sc * C::W3_CHUNK + (1 * 2 * C::CT + (t + e) * 16) * 16);
                }
            };
            ld_a(0, 0);
#pragma unroll
            for (int i = 0; i < NSTEP; ++i) {
                if (i + 1 < NSTEP) ld_a(i + 1, (i + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
                const int t = (2 * i) % C::NT3, ch = st * C::SC + (2 * i) / C::NT3;
                mma3x2(acc3[t], acc3[t + 1], a_hi[i & 1][0], a_lo[i & 1][0], a_hi[i & 1][1], a_lo[i & 1][1], xh[ch], xl[ch]);
                __builtin_amdgcn_sched_barrier(0);
            }
            stage_sync();
            sb ^= 1;
        }
        const float* tab = reinterpret_cast<const float*>(tabbuf + (j & 1) * C::TAB_BYTES);
#pragma unroll
        for (int u = 0; u < C::NU; ++u) {
            // ---- tiles 2 u, 2 u + 1 of the co-tile: scale back, + bias, + identity, ReLU, store, split: conv1's B fragment of k-step u -----------
            unsigned int hw[4], lw[4];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const int t = 2 * u + tt, co4 = 16 * t + 4 * kb;                      // (within the co-tile)
                const float4 sc = *reinterpret_cast<const float4*>(tab + co4);
                const float4 bv = *reinterpret_cast<const float4*>(tab + C::CT + co4);
                float v0 = __fmul_rn(acc3[t][0], sc.x), v1 = __fmul_rn(acc3[t][1], sc.y), v2 = __fmul_rn(acc3[t][2], sc.z), v3 = __fmul_rn(acc3[t][3], sc.w);
                v0 = relu_keep_nan(__fadd_rn(__fadd_rn(v0, bv.x), rres[4 * tt + 0]));
                v1 = relu_keep_nan(__fadd_rn(__fadd_rn(v1, bv.y), rres[4 * tt + 1]));
                v2 = relu_keep_nan(__fadd_rn(__fadd_rn(v2, bv.z), rres[4 * tt + 2]));
                v3 = relu_keep_nan(__fadd_rn(__fadd_rn(v3, bv.w), rres[4 * tt + 3]));
                if (pos_ok) {
                    char* yo = reinterpret_cast<char*>(p.y + (int64_t)(co_j + 16 * t) * V);       // (uniform; rows 4 kb .. are in lane_off)
                    *reinterpret_cast<float*>(yo + (size_t)lane_off) = v0;
                    *reinterpret_cast<float*>(yo + V * 4 + (size_t)lane_off) = v1;
                    *reinterpret_cast<float*>(yo + V * 8 + (size_t)lane_off) = v2;
                    *reinterpret_cast<float*>(yo + V * 12 + (size_t)lane_off) = v3;
                }
                split_pair_f16(v0, v1, hw[2 * tt], lw[2 * tt]);
                split_pair_f16(v2, v3, hw[2 * tt + 1], lw[2 * tt + 1]);
            }
            // The lane (n, rb) holds rows 4 rb + 0..3 of both tiles; conv1's k slots of lane (n, kb) are channels 8 kb + 0..7 of the 32 (the packed
            // weights' order: one conflict-free 16-byte read per fragment).  Two half / row exchanges per word move them: after permlane32_swap the
            // row blocks hold (T0 rb0, T0 rb1, T1 rb0, T1 rb1) | (T0 rb2, T0 rb3, T1 rb2, T1 rb3), after permlane16_swap (T0 rb0, T0 rb2, T1 rb0, T1 rb2) |
            // (T0 rb1, T0 rb3, T1 rb1, T1 rb3): row block kb now has (8 kb + 0..3 | 8 kb + 4..7).
            unsigned int bw[2][4];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const unsigned int t0 = pl ? lw[i] : hw[i], t1 = pl ? lw[2 + i] : hw[2 + i];
                    auto s32 = __builtin_amdgcn_permlane32_swap(t0, t1, false, false);
                    auto s16 = __builtin_amdgcn_permlane16_swap(s32[0], s32[1], false, false);
                    bw[pl][i] = s16[0];
                    bw[pl][2 + i] = s16[1];
                }
            const u32x4 bh = {bw[0][0], bw[0][1], bw[0][2], bw[0][3]}, bl = {bw[1][0], bw[1][1], bw[1][2], bw[1][3]};
            const f16x8 b_hi = __builtin_bit_cast(f16x8, bh), b_lo = __builtin_bit_cast(f16x8, bl);
            __builtin_amdgcn_sched_barrier(0);
            if (u + 1 < C::NU) { dma_w1(j * C::NU + u + 1, eb ^ 1); load_identity(co_j + 32 * (u + 1), rres); }
            else if (j + 1 < C::NCT) dma_w3(j + 1, 0, sb);
            else dma_tail_tab();
            __builtin_amdgcn_sched_barrier(0);
            // ---- conv1, k-step u ------------------------------------------------------------------------------------------------------------
            const char* w1b = w1buf + eb * C::W1_BYTES + (((kb >> 1) * 2 * 2 + (kb & 1)) * C::MID + n) * 16;      // row (g = kb / 2, plane 0, h = kb % 2)
            f16x8 a_hi[1][2], a_lo[1][2];
            auto ld_a1 = [&](const int i, const int k) __attribute__((always_inline)) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    a_hi[k][e] = *reinterpret_cast<const f16x8*>(w1b + (0 * 2 * C::MID + (2 * i + e) * 16) * 16);
                    a_lo[k][e] = *reinterpret_cast<const f16x8*>(w1b + (1 * 2 * C::MID + (2 * i + e) * 16) * 16);
                }
            };
#pragma unroll
            for (int i = 0; i < C::NT1 / 2; ++i) {
                ld_a1(i, 0);
                __builtin_amdgcn_sched_barrier(0);
                mma3x2(acc1[2 * i], acc1[2 * i + 1], a_hi[0][0], a_lo[0][0], a_hi[0][1], a_lo[0][1], b_hi, b_lo);
                __builtin_amdgcn_sched_barrier(0);
            }
            stage_sync();
            eb ^= 1;
        }
    }
    // ---- conv1's epilogue ------------------------------------------------------------------------------------------------------------------
    if (pos_ok) {
        const int hwp = p.dec_H * p.dec_W;
        const int t2 = pos / hwp, r2 = pos - t2 * hwp, y2 = r2 / p.dec_W, x2 = r2 - y2 * p.dec_W;
        const unsigned int z_off = (unsigned int)(((int64_t)(4 * kb) * p.z_cs + (int64_t)t2 * p.z_ts + (int64_t)y2 * p.z_ys + x2) * 4);      // bytes
        const float* ttab = reinterpret_cast<const float*>(w3buf);
#pragma unroll
        for (int m1 = 0; m1 < C::NT1; ++m1) {
            const int co4 = m1 * 16 + 4 * kb;
            const float4 sc = *reinterpret_cast<const float4*>(ttab + co4);
            const float4 bv = *reinterpret_cast<const float4*>(ttab + C::MID + co4);
            char* zo = reinterpret_cast<char*>(p.z + (int64_t)(m1 * 16) * p.z_cs);     // (uniform)
            *reinterpret_cast<float*>(zo + (size_t)z_off) = relu_keep_nan(__fadd_rn(__fmul_rn(acc1[m1][0], sc.x), bv.x));
            *reinterpret_cast<float*>(zo + p.z_cs * 4 + (size_t)z_off) = relu_keep_nan(__fadd_rn(__fmul_rn(acc1[m1][1], sc.y), bv.y));
            *reinterpret_cast<float*>(zo + p.z_cs * 8 + (size_t)z_off) = relu_keep_nan(__fadd_rn(__fmul_rn(acc1[m1][2], sc.z), bv.z));
            *reinterpret_cast<float*>(zo + p.z_cs * 12 + (size_t)z_off) = relu_keep_nan(__fadd_rn(__fmul_rn(acc1[m1][3], sc.w), bv.w));
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// The one-wave-per-SIMD form ("R1"; MID = 256).  The 16-column form above is latency-shaped: two 256-register waves per SIMD meet the same
// barrier 64 times, a stage is 0.7 us of matrix work behind LDS reads that one spare fragment set cannot cover, and every stage's vmcnt(0)
// also waits for the identity loads and output stores of that stage (PMC: waves parked 42 %, the MFMA pipe busy 29 % of the launch).  Here
// a workgroup is FOUR waves, one per SIMD, with the whole 512-register file each:
//   * a wave owns 32 positions and keeps, for all of them, conv3's whole input (MID / 16 k-groups x (hi, lo) = 128 registers, loaded once),
//     conv1's MID x 32 accumulators (128) and the co-tile's CT x 32 (64): an A fragment read from LDS feeds a 32-column MFMA, i.e. half the
//     LDS traffic per MFMA cycle of the 16-column form, and the k order per accumulator is the separate launches' (v_mfma_f32_32x32x16_f16,
//     two 16-deep k-groups per 32-channel chunk) => bit-identical to them again;
//   * the spare registers are a ring of A-fragment sets two steps ahead of the MFMAs, and a second identity buffer: the identity rows of a
//     32-channel tile are requested two stages before its epilogue;
//   * the end-of-stage wait is COUNTED: the stage's LDS-DMA pieces are issued first, so `s_waitcnt vmcnt(n)` with n = the identity loads
//     and output stores issued behind them waits for the weights only (vmcnt retires in issue order);
//   * the epilogue of tile u + 1 (scale / bias / identity / ReLU / store / split / lane exchange) is cut into slices that sit between the
//     MFMAs of conv1's k-step u; identity loads and output stores are buffer instructions (row base in an SGPR offset, one loop-invariant
//     lane offset; columns past V are dropped by the descriptor's range check): no address arithmetic, no branch inside a stage.
typedef __amdgpu_buffer_rsrc_t ft_rsrc_t;
#define FT_VMCNT_(n) __builtin_amdgcn_s_waitcnt(((n) & 15) | (((n) >> 4) << 14) | 0x0F70)
#define FT_VMCNT(n) FT_VMCNT_(n)
#define FT_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)

template <int MID_, int CT_, int DS_ = 0, int N1_ = MID_, bool LAT_ = false>
struct FusedTailR1Cfg {
    static constexpr int MID = MID_, CT = CT_, COUT = 4 * MID_;
    static constexpr int N1 = N1_;                            // output channels of the conv1 slot: the next block's conv1 (MID), or the stage's FPN lateral (256)
    static constexpr bool LAT = LAT_;                         // stage-end variant: the slot is the FPN lateral (no ReLU, dense map), and the kept quarter of y goes to p.xsub
    static constexpr int EST = LAT ? 32 : 16;                 // stores of one tile's epilogue: 16 rows of y, and their copies into p.xsub
    static constexpr int DS = DS_, NGD = DS_ / 16;           // shortcut variant: its input channels / k-groups (0: the identity comes from p.res)
    static constexpr int NW = 4, NTHREADS = 64 * NW, P = 32 * NW;
    static constexpr int NC3 = MID / 32, NG = MID / 16, NCT = COUT / CT;
    static constexpr int MI3 = CT / 32, MI1 = N1 / 32;         // 32-row accumulator tiles: conv3 co-tile, conv1 slot
    static constexpr int SC = 2;                              // conv3 chunks per stage
    static constexpr int NS = NC3 / SC, NU = CT / 32;         // conv3 stages / conv1 k-steps per co-tile
    static constexpr int NSD = DS / 32 / SC;                  // shortcut stages per co-tile
    static_assert(DS % (32 * SC) == 0, "shortcut: whole stages");
    static constexpr int NX3 = SC * 2 * (MI3 / 2), NX1 = 2 * (MI1 / 2);     // steps (two tiles x three products) per conv3 stage / conv1 k-step
    static constexpr int W3_CHUNK = 8 * CT * 16, W3_BYTES = SC * W3_CHUNK;
    static constexpr int W1_BYTES = 8 * N1 * 16;
    static_assert(W3_CHUNK == FT_WL.slab_bytes(CT, FT_WL.CK) && W1_BYTES == FT_WL.slab_bytes(N1, FT_WL.CK), "tile byte sizes follow the packed-weight layout");
    static constexpr int TAB_BYTES = 1024;
    static constexpr int LDS_BYTES = 2 * W3_BYTES + 2 * W1_BYTES + 2 * TAB_BYTES;
    static constexpr int W3_PIECES = W3_BYTES / 1024 / NW, W1_PIECES = W1_BYTES / 1024 / NW;
    // a conv1 k-step of NX1 steps carries the next tile's epilogue: SL slices (rows 8 q4 ..) per step from step S0 on, the lane exchanges behind them;
    // the requests of the next stage go out in the steps before S0, M_PPS pieces per step (MID = 256: 8 steps -- requests 0-1, slices 2-5, exchanges
    // 6-7; MID = 128: 4 steps -- requests 0, slices 1-2, exchanges 3)
    static constexpr int SL = 8 / NX1, S0 = NX1 / 4, M_PPS = 8 / S0;
    static_assert(NC3 % SC == 0 && MI3 % 2 == 0 && MI1 % 2 == 0 && W3_BYTES % (1024 * NW) == 0 && W1_BYTES % (1024 * NW) == 0 && 2 * CT * 4 <= TAB_BYTES, "whole DMA pieces per wave");
    static_assert(LDS_BYTES <= 160 * 1024 && 2 * N1 * 4 <= W3_BYTES && 16 + EST <= 63 && (NX1 == 8 || NX1 == 4) && NX3 == 8 && MI3 == 4 && NS >= 2 && NU >= 2 && NU % 2 == 0, "LDS / slice placement / identity buffer parity");
    static_assert(W3_PIECES == 8 && W1_PIECES <= 8, "the pieces of a stage are requested in its first steps");
    static_assert(NG * 8 + MI1 * 16 <= 256, "the conv3 input and conv1's accumulators are the AGPR half of the register file");
};

template <class C>
__global__ __launch_bounds__(C::NTHREADS, 1) void fused_tail_r1_kernel(const FusedTailParams p) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(1024))) char smem[C::LDS_BYTES];
    char* const w3buf = smem;
    char* const w1buf = smem + 2 * C::W3_BYTES;
    char* const tabbuf = smem + 2 * C::W3_BYTES + 2 * C::W1_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int pos = blockIdx.x * C::P + wave * 32 + l31;       // this lane's position (column of every accumulator tile of the wave)
    const bool pos_ok = pos < p.V;
    const int pos_c = min(pos, p.V - 1);
    const int64_t V = p.V;
    const unsigned int V4 = (unsigned int)p.V * 4u;           // bytes per channel row
    // rows (r & 3) + 8 (r >> 2) + 4 half of a 32-channel tile: the 4 half part and the column are the lane offset; loads of a column past V read
    // the last valid one, its stores carry an offset the descriptor's range check drops
    const unsigned int lane_ld = (unsigned int)(4 * half) * V4 + (unsigned int)pos_c * 4u;
    const unsigned int lane_st = pos_ok ? lane_ld : 0xFFFFFF00u;
    const unsigned int tile_bytes = (unsigned int)C::CT * V4;  // a co-tile's rows: the extent of its descriptors
    // stage-end variant: the kept quarter of y -- this lane's position is (t, y, x) of [T][dec_H][dec_W] planes, kept where y and x are even; every
    // other lane carries the offset the range check drops
    const unsigned int SV4 = C::LAT ? (unsigned int)p.sub_V * 4u : 0u;
    unsigned int lane_sub = 0xFFFFFF00u;
    if constexpr (C::LAT) {
        const int hwp = p.dec_H * p.dec_W, t2 = pos_c / hwp, r2 = pos_c - t2 * hwp, y2 = r2 / p.dec_W, x2 = r2 - y2 * p.dec_W;
        if (pos_ok && !((y2 | x2) & 1)) lane_sub = (unsigned int)(4 * half) * SV4 + (unsigned int)((t2 * (p.dec_H / 2) + y2 / 2) * (p.dec_W / 2) + x2 / 2) * 4u;
    }
    typedef __attribute__((address_space(3))) void* lptr_t;
    const float* inv3 = reinterpret_cast<const float*>(p.w3 + FT_WL.inv_offset(C::COUT, C::MID));
    const float* inv1 = reinterpret_cast<const float*>(p.w1 + FT_WL.inv_offset(C::N1, C::COUT));

    // ---- LDS-DMA, as inline assembly ---------------------------------------------------------------------------------------------------
    // One piece = 1 KB per wave instruction (global_load_lds_dwordx4: wave-uniform 64-bit base in SGPRs + ONE loop-invariant lane offset, LDS
    // base in M0).  Assembly, not the builtin: the compiler cannot tell an LDS read from the target of a DMA it knows to be in flight, and
    // guards the first table read behind a request with a vmcnt(0); requests it does not see are waited for by the counted s_waitcnt at the
    // end of the stage and by nothing else.  (Its own counts for the identity loads stay safe: unseen requests only make a vmcnt(n) stricter.)
    const unsigned int lane16 = (unsigned int)lane * 16u;
    const unsigned int lds_w3 = (unsigned int)(uintptr_t)(lptr_t)w3buf, lds_w1 = (unsigned int)(uintptr_t)(lptr_t)w1buf;
    auto dma_piece = [&](const char* sbase, const unsigned int lds_addr) __attribute__((always_inline)) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(lds_addr), "v"(lane16), "s"(sbase) : "memory");
    };
    auto dma_w3 = [&](const int j, const int st, const int buf, const int k) __attribute__((always_inline)) {      // piece k of chunks SC st .. of co-tile j
        constexpr int PER_ROW = C::CT * 16 / 1024, PER_CHUNK = C::W3_CHUNK / 1024;
        const int idx = wave + k * C::NW, sc = idx / PER_CHUNK, r = idx % PER_CHUNK, row = r / PER_ROW, part = r % PER_ROW;
        dma_piece(p.w3 + ((int64_t)(st * C::SC + sc) * 8 + row) * (C::COUT * 16) + (int64_t)j * (C::CT * 16) + part * 1024, lds_w3 + buf * C::W3_BYTES + idx * 1024);
    };
    auto dma_wd = [&](const int j, const int st, const int buf, const int k) __attribute__((always_inline)) {      // the same piece of the shortcut's blob ([..][4 MID][16 B] too)
        constexpr int PER_ROW = C::CT * 16 / 1024, PER_CHUNK = C::W3_CHUNK / 1024;
        const int idx = wave + k * C::NW, sc = idx / PER_CHUNK, r = idx % PER_CHUNK, row = r / PER_ROW, part = r % PER_ROW;
        dma_piece(p.wd + ((int64_t)(st * C::SC + sc) * 8 + row) * (C::COUT * 16) + (int64_t)j * (C::CT * 16) + part * 1024, lds_w3 + buf * C::W3_BYTES + idx * 1024);
    };
    auto dma_w1 = [&](const int cc, const int buf, const int k) __attribute__((always_inline)) {                   // piece k of conv1 k-step (32-channel chunk) cc
        const int idx = wave + k * C::NW;
        dma_piece(p.w1 + (int64_t)cc * C::W1_BYTES + (int64_t)idx * 1024, lds_w1 + buf * C::W1_BYTES + idx * 1024);
    };
    // co-tile j's (1 / scale | bias) table: lanes 0 .. CT / 4 - 1 of wave 0 fetch the scales, the next CT / 4 the biases (an ordinary load at the
    // top of conv3's last stage), and store them at its end
    float4 tabv = {0.f, 0.f, 0.f, 0.f};
    auto tab_fetch = [&](const int j) __attribute__((always_inline)) {
        if (wave == 0 && lane < 2 * (C::CT / 4))
            tabv = *reinterpret_cast<const float4*>((lane < C::CT / 4 ? inv3 : p.b3 - C::CT) + (int64_t)j * C::CT + lane * 4);
    };
    auto tab_store = [&](const int j) __attribute__((always_inline)) {
        if (wave == 0 && lane < 2 * (C::CT / 4)) *reinterpret_cast<float4*>(tabbuf + (j & 1) * C::TAB_BYTES + lane * 16) = tabv;
    };
    // shortcut variant: the shortcut's table of co-tile j goes to the OTHER table buffer -- co-tile j - 1's, idle since the barrier behind its last
    // k-step -- in the shortcut's first stage, and is consumed behind its last one (co-tile j's own table is stored while waves may still be there)
    constexpr bool DSV = C::DS > 0;
    float4 tabdv = {0.f, 0.f, 0.f, 0.f};
    auto tabd_fetch = [&](const int j) __attribute__((always_inline)) {
        const float* invd = reinterpret_cast<const float*>(p.wd + FT_WL.inv_offset(C::COUT, C::DS));
        if (wave == 0 && lane < 2 * (C::CT / 4))
            tabdv = *reinterpret_cast<const float4*>((lane < C::CT / 4 ? invd : p.bd - C::CT) + (int64_t)j * C::CT + lane * 4);
    };
    auto tabd_store = [&](const int j) __attribute__((always_inline)) {
        if (wave == 0 && lane < 2 * (C::CT / 4)) *reinterpret_cast<float4*>(tabbuf + ((j + 1) & 1) * C::TAB_BYTES + lane * 16) = tabdv;
    };
    auto rsrc_of = [&](const float* base, const int jj) __attribute__((always_inline)) {        // the CT rows of co-tile jj of a dense [4 MID][V] map
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + (int64_t)jj * C::CT * V), 0, (int)tile_bytes, 0x00020000);
    };
    // identity rows of 32-channel tile u of co-tile jj, this lane's column
    auto load_identity = [&](const int jj, const int u, float (&rr)[16]) __attribute__((always_inline)) {
        const ft_rsrc_t rs = rsrc_of(p.res, jj);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            rr[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, lane_ld, (unsigned int)(32 * u + (r & 3) + 8 * (r >> 2)) * V4, 0));
    };
    const f16x8 k2048 = {(_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE),
                         (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE), (_Float16)(1.0f / F16X3_LO_SCALE)};
    // two tiles per step, their MFMAs alternating (never two in a row on one accumulator); per accumulator the three products in mma3's order
    auto mma6 = [&](f32x16& c0, f32x16& c1, const f16x8 (&a_hi)[2], const f16x8 (&a_lo)[2], const f16x8 (&a_his)[2], const f16x8 b_hi, const f16x8 b_lo)
        __attribute__((always_inline)) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo[0], b_hi, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo[1], b_hi, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_his[0], b_lo, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_his[1], b_lo, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[0], b_hi, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[1], b_hi, c1, 0, 0, 0);
    };

    // ---- prologue: the first stage's weights, the first two tiles' identity rows, the wave's whole conv3 input --------------------------
#pragma unroll
    for (int k = 0; k < C::W3_PIECES; ++k) {
        if constexpr (DSV) dma_wd(0, 0, 0, k);
        else dma_w3(0, 0, 0, k);
    }
    float rres[2][16];
    if constexpr (!DSV) {
        load_identity(0, 0, rres[0]);
        load_identity(0, 1, rres[1]);
    }
    f16x8 xh[C::NG], xl[C::NG];                    // k-group G: lane (half, n) = octet 2 G + half of both planes at its position
    {
        const char* xs = reinterpret_cast<const char*>(p.x16) + (size_t)((unsigned int)pos_c * 16u);
#pragma unroll
        for (int G = 0; G < C::NG; ++G) {
            xh[G] = *reinterpret_cast<const f16x8*>(xs + ((int64_t)(2 * G + half)) * V * 16);
            xl[G] = *reinterpret_cast<const f16x8*>(xs + ((int64_t)(C::MID / 8 + 2 * G + half)) * V * 16);
        }
    }
    // shortcut variant: the wave's whole shortcut input too, fp32 in, split here -- k-group G, lane (half, n): channels 16 G + 8 half + 0 .. 7 at its
    // position, the packed weights' k order (buffer loads: the channel row is an SGPR offset)
    f16x8 xdh[DSV ? C::NGD : 1], xdl[DSV ? C::NGD : 1];
    if constexpr (DSV) {
        const ft_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.xs), 0, (int)((unsigned int)C::DS * V4), 0x00020000);
        const unsigned int lane_xs = (unsigned int)(8 * half) * V4 + (unsigned int)pos_c * 4u;
#pragma unroll
        for (int G = 0; G < C::NGD; ++G) {
            float xr[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) xr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, lane_xs, (unsigned int)(16 * G + i) * V4, 0));
            u32x4 hw4, lw4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned int hwd, lwd;
                split_pair_f16(xr[2 * i], xr[2 * i + 1], hwd, lwd);
                hw4[i] = hwd; lw4[i] = lwd;
            }
            xdh[G] = __builtin_bit_cast(f16x8, hw4);
            xdl[G] = __builtin_bit_cast(f16x8, lw4);
        }
    }
    f32x16 acc1[C::MI1];
#pragma unroll
    for (int m = 0; m < C::MI1; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[m][r] = 0.f;
    FT_VMCNT(0);
    __syncthreads();
    int sb = 0, eb = 0;                                      // buffers of the conv3 stage / the conv1 k-step about to run
#pragma unroll 1
    for (int j = 0; j < C::NCT; ++j) {
        // ---- shortcut variant: NSD stages of SC chunks of the shortcut (weights through the w3 buffers, steps as in conv3's stages) in front of conv3's;
        // the last one requests conv3's first stage.  Scale and bias behind them: accd then holds what the stand-alone launch would have written
        // to the shortcut map, and the epilogue slices add it where they otherwise add the loaded identity rows.
        f32x16 accd[DSV ? C::MI3 : 1];
        if constexpr (DSV) {
#pragma unroll
            for (int m = 0; m < C::MI3; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) accd[m][r] = 0.f;
#pragma unroll
            for (int st = 0; st < C::NSD; ++st) {
                if (st == 0) tabd_fetch(j);
                const char* wb = w3buf + sb * C::W3_BYTES + (half * C::CT + l31) * 16;
                f16x8 a_hi[3][2], a_lo[3][2], a_his[2][2];
                auto ld3 = [&](const int s, const int k) __attribute__((always_inline)) {
                    const int mp = s / (2 * C::SC), sc = (s % (2 * C::SC)) / 2, g = s % 2;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        a_hi[k][e] = *reinterpret_cast<const f16x8*>(wb + sc * C::W3_CHUNK + (((g * 2 + 0) * 2) * C::CT + (2 * mp + e) * 32) * 16);
                        a_lo[k][e] = *reinterpret_cast<const f16x8*>(wb + sc * C::W3_CHUNK + (((g * 2 + 1) * 2) * C::CT + (2 * mp + e) * 32) * 16);
                    }
                };
                ld3(0, 0);
                ld3(1, 1);
                a_his[0][0] = a_hi[0][0] * k2048;
                a_his[0][1] = a_hi[0][1] * k2048;
#pragma unroll
                for (int s = 0; s < C::NX3; ++s) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (s < 2) {
#pragma unroll
                        for (int k = 4 * s; k < 4 * s + 4; ++k) {
                            if (st + 1 < C::NSD) dma_wd(j, st + 1, sb ^ 1, k);
                            else dma_w3(j, 0, sb ^ 1, k);
                        }
                    }
                    if (s + 2 < C::NX3) ld3(s + 2, (s + 2) % 3);
                    if (s + 1 < C::NX3) {
                        a_his[(s + 1) & 1][0] = a_hi[(s + 1) % 3][0] * k2048;
                        a_his[(s + 1) & 1][1] = a_hi[(s + 1) % 3][1] * k2048;
                    }
                    const int mp = s / (2 * C::SC), sc = (s % (2 * C::SC)) / 2, g = s % 2, G = 2 * (st * C::SC + sc) + g;
                    mma6(accd[2 * mp], accd[2 * mp + 1], a_hi[s % 3], a_lo[s % 3], a_his[s & 1], xdh[G], xdl[G]);
#pragma unroll
                    for (int i = 0; i < 6; ++i) { FT_SGB(0x008, 1); FT_SGB(0x100, 1); FT_SGB(0x002, 2); }
                }
                __builtin_amdgcn_sched_barrier(0);
                FT_VMCNT(0);                                 // (nothing was issued behind the requests)
                if (st == 0) tabd_store(j);
                __syncthreads();
                sb ^= 1;
            }
            const float* tabd = reinterpret_cast<const float*>(tabbuf + ((j + 1) & 1) * C::TAB_BYTES) + 4 * half;
#pragma unroll
            for (int u = 0; u < C::MI3; ++u)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const float4 sc = *reinterpret_cast<const float4*>(tabd + 32 * u + 8 * q4);
                    const float4 bv = *reinterpret_cast<const float4*>(tabd + C::CT + 32 * u + 8 * q4);
                    accd[u][4 * q4 + 0] = __fadd_rn(__fmul_rn(accd[u][4 * q4 + 0], sc.x), bv.x);
                    accd[u][4 * q4 + 1] = __fadd_rn(__fmul_rn(accd[u][4 * q4 + 1], sc.y), bv.y);
                    accd[u][4 * q4 + 2] = __fadd_rn(__fmul_rn(accd[u][4 * q4 + 2], sc.z), bv.z);
                    accd[u][4 * q4 + 3] = __fadd_rn(__fmul_rn(accd[u][4 * q4 + 3], sc.w), bv.w);
                }
            // (pinned here: sunk to the slices that read them, these sums would leave the whole table live in registers across conv3's stages)
#pragma unroll
            for (int u = 0; u < C::MI3; ++u) asm volatile("" : "+v"(accd[u]));
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x16 acc3[C::MI3];
#pragma unroll
        for (int m = 0; m < C::MI3; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc3[m][r] = 0.f;
        // ---- the epilogue's pieces (used from conv3's last stage on) -----------------------------------------------------------------------
        const float* tab = reinterpret_cast<const float*>(tabbuf + (j & 1) * C::TAB_BYTES) + 4 * half;
        const ft_rsrc_t ry = rsrc_of(p.y, j);
        const ft_rsrc_t rsub = __builtin_amdgcn_make_buffer_rsrc(C::LAT ? p.xsub + (int64_t)j * C::CT * p.sub_V : p.y, 0, (int)((unsigned int)C::CT * SV4), 0x00020000);
        unsigned int hw[8], lw[8];
        f16x8 b_hi[2][2], b_lo[2][2];                       // [k-step parity][k-group]: conv1's B fragments
        // rows 8 q4 + 4 half + 0 .. 3 of tile u: scale back, + bias, + identity, ReLU, store, split
        auto e_slice = [&](const int u, const int q4) __attribute__((always_inline)) {
            const int c4 = 32 * u + 8 * q4;
            const float4 sc = *reinterpret_cast<const float4*>(tab + c4);
            const float4 bv = *reinterpret_cast<const float4*>(tab + C::CT + c4);
            float rr[4];                                    // the identity: loaded rows, or the shortcut's finished sums
#pragma unroll
            for (int i = 0; i < 4; ++i) rr[i] = DSV ? accd[DSV ? u : 0][4 * q4 + i] : rres[u & 1][4 * q4 + i];
            // (explicitly rounded steps: the standalone kernel scales its accumulators in one place and adds bias / identity in another)
            float v0 = __fmul_rn(acc3[u][4 * q4 + 0], sc.x), v1 = __fmul_rn(acc3[u][4 * q4 + 1], sc.y), v2 = __fmul_rn(acc3[u][4 * q4 + 2], sc.z),
                  v3 = __fmul_rn(acc3[u][4 * q4 + 3], sc.w);
            v0 = relu_keep_nan(__fadd_rn(__fadd_rn(v0, bv.x), rr[0]));
            v1 = relu_keep_nan(__fadd_rn(__fadd_rn(v1, bv.y), rr[1]));
            v2 = relu_keep_nan(__fadd_rn(__fadd_rn(v2, bv.z), rr[2]));
            v3 = relu_keep_nan(__fadd_rn(__fadd_rn(v3, bv.w), rr[3]));
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v0), ry, lane_st, (unsigned int)(c4 + 0) * V4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v1), ry, lane_st, (unsigned int)(c4 + 1) * V4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v2), ry, lane_st, (unsigned int)(c4 + 2) * V4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v3), ry, lane_st, (unsigned int)(c4 + 3) * V4, 0);
            if constexpr (C::LAT) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v0), rsub, lane_sub, (unsigned int)(c4 + 0) * SV4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v1), rsub, lane_sub, (unsigned int)(c4 + 1) * SV4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v2), rsub, lane_sub, (unsigned int)(c4 + 2) * SV4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v3), rsub, lane_sub, (unsigned int)(c4 + 3) * SV4, 0);
            }
            split_pair_f16(v0, v1, hw[2 * q4], lw[2 * q4]);
            split_pair_f16(v2, v3, hw[2 * q4 + 1], lw[2 * q4 + 1]);
        };
        // k-group gg of the tile as conv1's B fragment: the lane halves hold (q4 even: ch 0-3 | 4-7), (q4 odd: 8-11 | 12-15) of the group; swapping
        // the upper half of the q4-even words with the lower half of the q4-odd words gives (0-3, 4-7) to half 0 and (8-11, 12-15) to half 1
        auto e_perm = [&](const int gg, f16x8& bh, f16x8& bl) __attribute__((always_inline)) {
            unsigned int xh_[2], yh_[2], xl_[2], yl_[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                auto sh = __builtin_amdgcn_permlane32_swap(hw[4 * gg + i], hw[4 * gg + 2 + i], false, false);
                xh_[i] = sh[0]; yh_[i] = sh[1];
                auto sl = __builtin_amdgcn_permlane32_swap(lw[4 * gg + i], lw[4 * gg + 2 + i], false, false);
                xl_[i] = sl[0]; yl_[i] = sl[1];
            }
            const u32x4 bh4 = {xh_[0], xh_[1], yh_[0], yh_[1]}, bl4 = {xl_[0], xl_[1], yl_[0], yl_[1]};
            bh = __builtin_bit_cast(f16x8, bh4);
            bl = __builtin_bit_cast(f16x8, bl4);
        };
        // ---- conv3: NS stages of SC chunks ------------------------------------------------------------------------------------------------
#pragma unroll
        for (int st = 0; st < C::NS; ++st) {
            if (st + 2 == C::NS) tab_fetch(j);
            const char* wb = w3buf + sb * C::W3_BYTES + (half * C::CT + l31) * 16;
            f16x8 a_hi[3][2], a_lo[3][2], a_his[2][2];
            auto ld3 = [&](const int s, const int k) __attribute__((always_inline)) {
                const int mp = s / (2 * C::SC), sc = (s % (2 * C::SC)) / 2, g = s % 2;      // tile pair outermost: tiles 0-1 are finished half a stage early
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    a_hi[k][e] = *reinterpret_cast<const f16x8*>(wb + sc * C::W3_CHUNK + (((g * 2 + 0) * 2) * C::CT + (2 * mp + e) * 32) * 16);
                    a_lo[k][e] = *reinterpret_cast<const f16x8*>(wb + sc * C::W3_CHUNK + (((g * 2 + 1) * 2) * C::CT + (2 * mp + e) * 32) * 16);
                }
            };
            ld3(0, 0);
            ld3(1, 1);
            a_his[0][0] = a_hi[0][0] * k2048;
            a_his[0][1] = a_hi[0][1] * k2048;
#pragma unroll
            for (int s = 0; s < C::NX3; ++s) {
                __builtin_amdgcn_sched_barrier(0);
                if (s < 2) {                                 // what the next stage reads, four pieces in each of the first two steps
#pragma unroll
                    for (int k = 4 * s; k < 4 * s + 4; ++k) {
                        if (st + 1 < C::NS) dma_w3(j, st + 1, sb ^ 1, k);
                        else if (k < C::W1_PIECES) dma_w1(j * C::NU, eb, k);
                    }
                }
                if (s + 2 < C::NX3) ld3(s + 2, (s + 2) % 3);
                if (s + 1 < C::NX3) {
                    a_his[(s + 1) & 1][0] = a_hi[(s + 1) % 3][0] * k2048;
                    a_his[(s + 1) & 1][1] = a_hi[(s + 1) % 3][1] * k2048;
                }
                // the co-tile's LAST stage: tile 0 got its last products in step NX3 / 2 - 1 -- its epilogue, a slice per step, sits between the MFMAs of
                // the other tile pair (nothing of it is left in front of conv1's first k-step but the two lane exchanges)
                if (st + 1 == C::NS && s >= C::NX3 / 2) e_slice(0, s - C::NX3 / 2);
                const int mp = s / (2 * C::SC), sc = (s % (2 * C::SC)) / 2, g = s % 2, G = 2 * (st * C::SC + sc) + g;
                mma6(acc3[2 * mp], acc3[2 * mp + 1], a_hi[s % 3], a_lo[s % 3], a_his[s & 1], xh[G], xl[G]);
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    FT_SGB(0x008, 1); FT_SGB(0x100, 1);
                    if (st + 1 == C::NS && s >= C::NX3 / 2) { FT_SGB(0x002, 7); FT_SGB(0x040, C::LAT ? 2 : 1); }
                    else FT_SGB(0x002, 2);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (st + 1 == C::NS) FT_VMCNT(C::EST);           // (tile 0's output stores stay in flight; otherwise nothing was issued behind the requests)
            else FT_VMCNT(0);
            if (st + 2 == C::NS) tab_store(j);
            __syncthreads();
            sb ^= 1;
        }
        // ---- conv1's k-steps, each carrying the next tile's epilogue ---------------------------------------------------------------------------
        e_perm(0, b_hi[0][0], b_lo[0][0]);
        e_perm(1, b_hi[0][1], b_lo[0][1]);
#pragma unroll
        for (int u = 0; u < C::NU; ++u) {
            const char* w1b = w1buf + eb * C::W1_BYTES + (half * C::N1 + l31) * 16;
            f16x8 a_hi[3][2], a_lo[3][2], a_his[2][2];
            auto ld1 = [&](const int s, const int k) __attribute__((always_inline)) {
                const int g = s / (C::MI1 / 2), mp = s % (C::MI1 / 2);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    a_hi[k][e] = *reinterpret_cast<const f16x8*>(w1b + (((g * 2 + 0) * 2) * C::N1 + (2 * mp + e) * 32) * 16);
                    a_lo[k][e] = *reinterpret_cast<const f16x8*>(w1b + (((g * 2 + 1) * 2) * C::N1 + (2 * mp + e) * 32) * 16);
                }
            };
            ld1(0, 0);
            ld1(1, 1);
            a_his[0][0] = a_hi[0][0] * k2048;
            a_his[0][1] = a_hi[0][1] * k2048;
#pragma unroll
            for (int s = 0; s < C::NX1; ++s) {
                __builtin_amdgcn_sched_barrier(0);
                // Steps before S0: what the next stage reads.  Step S0: the identity rows of tile u + 2 (tile u's buffer: its epilogue ran a stage ago) --
                // a stage ahead of the slices that add them, and BEHIND this stage's requests, so that the counted wait leaves them in flight.
                // From step S0: the next tile's epilogue, SL slices (rows 8 q4 ..) per step; behind them its two lane exchanges.
                if (s < C::S0) {
#pragma unroll
                    for (int k = C::M_PPS * s; k < C::M_PPS * s + C::M_PPS; ++k) {
                        if (u + 1 < C::NU) { if (k < C::W1_PIECES) dma_w1(j * C::NU + u + 1, eb ^ 1, k); }
                        else if (j + 1 < C::NCT) { if constexpr (DSV) dma_wd(j + 1, 0, sb, k); else dma_w3(j + 1, 0, sb, k); }
                    }
                }
                if (!DSV && s == C::S0) load_identity(u + 2 < C::NU ? j : min(j + 1, C::NCT - 1), (u + 2) % C::NU, rres[u & 1]);      // (past the last tile: the last co-tile's rows again, never used)
                if (s + 2 < C::NX1) ld1(s + 2, (s + 2) % 3);
                if (s + 1 < C::NX1) {
                    a_his[(s + 1) & 1][0] = a_hi[(s + 1) % 3][0] * k2048;
                    a_his[(s + 1) & 1][1] = a_hi[(s + 1) % 3][1] * k2048;
                }
                if (u + 1 < C::NU) {
                    constexpr int SE = C::S0 + 4 / C::SL;     // first step behind the slices
                    if (s >= C::S0 && s < SE) {
#pragma unroll
                        for (int q = 0; q < C::SL; ++q) e_slice(u + 1, (s - C::S0) * C::SL + q);
                    }
                    if (C::SL == 1 ? s == SE : s == SE) e_perm(0, b_hi[(u + 1) & 1][0], b_lo[(u + 1) & 1][0]);
                    if (C::SL == 1 ? s == SE + 1 : s == SE) e_perm(1, b_hi[(u + 1) & 1][1], b_lo[(u + 1) & 1][1]);
                }
                const int g = s / (C::MI1 / 2), mp = s % (C::MI1 / 2);
                mma6(acc1[2 * mp], acc1[2 * mp + 1], a_hi[s % 3], a_lo[s % 3], a_his[s & 1], b_hi[u & 1][g], b_lo[u & 1][g]);
#pragma unroll
                for (int i = 0; i < 6; ++i) { FT_SGB(0x008, 1); FT_SGB(0x100, 1); FT_SGB(0x002, 7 * C::SL); FT_SGB(0x040, C::SL * (C::LAT ? 2 : 1)); FT_SGB(0x020, 3); }
            }
            __builtin_amdgcn_sched_barrier(0);
            // behind the requests of steps 0-1 this stage issued 16 identity loads and, if it carried an epilogue, its EST output stores: those stay in flight
            // (shortcut variant: no identity loads -- only the epilogue's stores, if any, are behind the requests)
            if (u + 1 < C::NU) FT_VMCNT(DSV ? C::EST : 16 + C::EST);
            else FT_VMCNT(DSV ? 0 : 16);
            __syncthreads();
            eb ^= 1;
        }
    }
    // ---- conv1's epilogue: scale back, + bias, ReLU, flat position -> (t, y, x) of the zero-haloed consumer layout -------------------------
    // its (1 / scale | bias) table: waves 0 / 1 put the MID scales / biases into the (idle) w3 buffer
    static_assert(C::N1 / 4 <= 64, "one lane per four channels");
    if (wave < 2 && lane < C::N1 / 4)
        *reinterpret_cast<float4*>(w3buf + wave * (C::N1 * 4) + lane * 16) = *reinterpret_cast<const float4*>((wave == 0 ? inv1 : p.b1) + lane * 4);
    __syncthreads();
    if (pos_ok) {
        const int hwp = p.dec_H * p.dec_W;
        const int t2 = pos / hwp, r2 = pos - t2 * hwp, y2 = r2 / p.dec_W, x2 = r2 - y2 * p.dec_W;
        const unsigned int z_off = (unsigned int)(((int64_t)(4 * half) * p.z_cs + (int64_t)t2 * p.z_ts + (int64_t)y2 * p.z_ys + x2) * 4);      // bytes
        const float* ttab = reinterpret_cast<const float*>(w3buf);
#pragma unroll
        for (int m1 = 0; m1 < C::MI1; ++m1)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co4 = m1 * 32 + 8 * q + 4 * half;
                const float4 sc = *reinterpret_cast<const float4*>(ttab + co4);
                const float4 bv = *reinterpret_cast<const float4*>(ttab + C::N1 + co4);
                char* zo = reinterpret_cast<char*>(p.z + (int64_t)(m1 * 32 + 8 * q) * p.z_cs);     // (uniform)
                *reinterpret_cast<float*>(zo + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 0], sc.x), bv.x));
                *reinterpret_cast<float*>(zo + p.z_cs * 4 + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 1], sc.y), bv.y));
                *reinterpret_cast<float*>(zo + p.z_cs * 8 + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 2], sc.z), bv.z));
                *reinterpret_cast<float*>(zo + p.z_cs * 12 + (size_t)z_off) = slot_act<C::LAT>(__fadd_rn(__fmul_rn(acc1[m1][4 * q + 3], sc.w), bv.w));
            }
    }
}

template <class C>
static int launch_fused_r1_cfg(const FusedTailParams& p, hipStream_t s) {
    const double flops = 2.0 * 2.0 * (double)C::MID * C::COUT * (double)p.V;
    void* ev = profile_begin(19, flops, s);
    hipLaunchKernelGGL(fused_tail_r1_kernel<C>, dim3((unsigned)ceil_div(p.V, C::P)), dim3(C::NTHREADS), 0, s, p);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

template <class C>
static int launch_fused16_cfg(const FusedTailParams& p, hipStream_t s) {
    const double flops = 2.0 * 2.0 * (double)C::MID * C::COUT * (double)p.V;
    void* ev = profile_begin(19, flops, s);
    hipLaunchKernelGGL(fused_tail16_kernel<C>, dim3((unsigned)ceil_div(p.V, C::P)), dim3(C::NTHREADS), 0, s, p);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

template <class C>
static int launch_fused_cfg(const FusedTailParams& p, hipStream_t s) {
    const double flops = 2.0 * 2.0 * (double)C::MID * C::COUT * (double)p.V;        // both GEMMs
    void* ev = profile_begin(19, flops, s);
    hipLaunchKernelGGL(fused_tail_kernel<C>, dim3((unsigned)ceil_div(p.V, C::P)), dim3(C::NTHREADS), 0, s, p);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

// stage-end variants: conv3 + the stage's FPN lateral; both GEMMs count, under a profile slot of their own
constexpr int FT_STAGE_END_TAG = 52;
template <class C, class K>
static int launch_stage_end_cfg(K kernel, const FusedTailParams& p, hipStream_t s) {
    const double flops = 2.0 * ((double)C::MID + C::N1) * C::COUT * (double)p.V;
    void* ev = profile_begin(FT_STAGE_END_TAG, flops, s);
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(p.V, C::P)), dim3(C::NTHREADS), 0, s, p);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

// (the kernel reads the two-plane f16x3 weight packing)
bool fused_tail_supported(int mid) { return mid == 64 || mid == 128 || mid == 256; }

// the shortcut variants: stage 1 (32-column form, 64 -> 256) and stage 2 (one wave per SIMD, 256 -> 512); one buffer descriptor spans the shortcut's input map
bool fused_shortcut_supported(int mid, int cin, int64_t V) {
    return ((mid == 64 && cin == 64) || (mid == 128 && cin == 256)) && (int64_t)cin * V * 4 < (1ll << 32) - (1 << 20) && (int64_t)128 * V * 4 < (1ll << 32) - (1 << 20);
}

// Stage-end variants (the last block of stages 1-3): the conv1 slot computes the stage's FPN lateral (1x1, 4 MID -> 256, + bias, no ReLU) into a
// dense [256][V] map, and the kept quarter of the block output goes to xsub.  One buffer descriptor spans a co-tile of y.
bool fused_stage_end_supported(int mid, int64_t V) {
    return (mid == 64 || mid == 128 || mid == 256) && V > 0 && V <= (1ll << 27) && (int64_t)128 * V * 4 < (1ll << 32) - (1 << 20);
}

int launch_fused_stage_end(int mid, const unsigned int* x16, const float* w3, const float* b3, const float* res, float* y, const float* wl, const float* bl,
                           float* lat, float* xsub, int T, int h, int w, hipStream_t s) {
    const int64_t V = (int64_t)T * h * w;
    SS_CHECK_ARG(x16 && w3 && b3 && res && y && wl && bl && lat && xsub, "fused_stage_end: null pointer");
    SS_CHECK_ARG(T > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && fused_stage_end_supported(mid, V), "fused_stage_end: mid = %d, %d planes of %d x %d (even)", mid, T, h, w);
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(x16) % 16 == 0 && reinterpret_cast<uintptr_t>(w3) % 16 == 0 && reinterpret_cast<uintptr_t>(wl) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(b3) % 16 == 0 && reinterpret_cast<uintptr_t>(bl) % 16 == 0, "fused_stage_end: 16-byte aligned operands");
    FusedTailParams p;
    p.x16 = x16; p.w3 = reinterpret_cast<const char*>(w3); p.b3 = b3; p.res = res; p.y = y;
    p.w1 = reinterpret_cast<const char*>(wl); p.b1 = bl;
    p.z = lat; p.z_cs = V; p.z_ts = (int64_t)h * w; p.z_ys = w; p.dec_H = h; p.dec_W = w;       // (the dense map, through the slot's (t, y, x) epilogue)
    p.V = (int)V;
    p.xs = nullptr; p.wd = nullptr; p.bd = nullptr;
    p.xsub = xsub; p.sub_V = (int)((int64_t)T * (h / 2) * (w / 2));
    if (mid == 256) { using C = FusedTailR1Cfg<256, 128, 0, 256, true>; return launch_stage_end_cfg<C>(fused_tail_r1_kernel<C>, p, s); }
    if (mid == 128) { using C = FusedTailR1Cfg<128, 128, 0, 256, true>; return launch_stage_end_cfg<C>(fused_tail_r1_kernel<C>, p, s); }
    // stage 1 (MID = 64 is one conv3 stage of the one-wave-per-SIMD form, which needs two): the 32-column form with a 64-channel co-tile -- 128 + 32
    // accumulator registers, 80 KB of LDS, two workgroups per CU
    using C = FusedTailCfg<64, 64, 128, 0, 256, true>;
    return launch_stage_end_cfg<C>(fused_tail_kernel<C>, p, s);
}

int launch_fused_tail(int mid, const unsigned int* x16, const float* w3, const float* b3, const float* res, float* y, const float* w1, const float* b1,
                      const StemsegVolume& z, int dec_H, int dec_W, int64_t V, int form, hipStream_t s, const float* ds_x, int ds_cin, const float* ds_w,
                      const float* ds_b) {
    SS_CHECK_ARG(x16 && w3 && b3 && y && w1 && b1 && z.ptr, "fused_tail: null pointer");
    // the identity: a dense map, or (ds_x) the block's projection shortcut computed in the kernel from the block's input
    SS_CHECK_ARG(ds_x ? (!res && ds_w && ds_b && fused_shortcut_supported(mid, ds_cin, V) && reinterpret_cast<uintptr_t>(ds_w) % 16 == 0 && reinterpret_cast<uintptr_t>(ds_b) % 16 == 0)
                      : res != nullptr, "fused_tail: identity map, or a shortcut (mid %d, %d input channels) this library has a kernel for", mid, ds_cin);
    SS_CHECK_ARG(fused_tail_supported(mid), "fused_tail: mid = %d (64, 128 or 256)", mid);
    SS_CHECK_ARG(V > 0 && V <= (1ll << 27) && z.c_stride <= (1ll << 27) && dec_H > 0 && dec_W > 0 && V % ((int64_t)dec_H * dec_W) == 0, "fused_tail: V = %lld positions of %d x %d planes",
                 (long long)V, dec_H, dec_W);
    SS_CHECK_ARG(z.C == mid, "fused_tail: consumer volume has %d channels, conv1 makes %d", z.C, mid);
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(x16) % 16 == 0 && reinterpret_cast<uintptr_t>(w3) % 16 == 0 && reinterpret_cast<uintptr_t>(w1) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(b3) % 16 == 0 && reinterpret_cast<uintptr_t>(b1) % 16 == 0, "fused_tail: 16-byte aligned operands");
    FusedTailParams p;
    p.x16 = x16; p.w3 = reinterpret_cast<const char*>(w3); p.b3 = b3; p.res = res; p.y = y;
    p.w1 = reinterpret_cast<const char*>(w1); p.b1 = b1;
    p.z = z.ptr; p.z_cs = z.c_stride; p.z_ts = z.t_stride; p.z_ys = z.y_stride; p.dec_H = dec_H; p.dec_W = dec_W;
    p.V = (int)V;
    p.xs = ds_x; p.wd = reinterpret_cast<const char*>(ds_w); p.bd = ds_b;
    p.xsub = nullptr; p.sub_V = 0;
    if (ds_x && mid == 128) return launch_fused_r1_cfg<FusedTailR1Cfg<128, 128, 256>>(p, s);
    if (ds_x) return launch_fused_cfg<FusedTailCfg<64, 128, 128, 64>>(p, s);
    if (mid == 256) {
        // form: 0 = the library's choice (the one-wave-per-SIMD form wherever its co-tile descriptors -- 128 V 4 bytes -- fit), 1 = the 16-column form, 2 = the
        // one-wave-per-SIMD form
        const bool r1_fits = (int64_t)128 * V * 4 < (1ll << 32) - (1 << 20);
        if (form != 1 && r1_fits) return launch_fused_r1_cfg<FusedTailR1Cfg<256, 128>>(p, s);
        return launch_fused16_cfg<FusedTail16Cfg<256>>(p, s);
    }
    if (mid == 128 && form != 1 && (int64_t)128 * V * 4 < (1ll << 32) - (1 << 20)) return launch_fused_r1_cfg<FusedTailR1Cfg<128, 128>>(p, s);
    // co-tile of the 32-column form (stages 1-2): 128 channels halve the re-reads of the input tile (229 / 196 registers, 80 / 72 KB: still two workgroups per CU); stage 2 335 -> 303 us, stage 1 510 -> 495
    if (mid == 128) return launch_fused_cfg<FusedTailCfg<128, 128, 128>>(p, s);
    return launch_fused_cfg<FusedTailCfg<64, 128, 128>>(p, s);
}

}  // namespace stemseg
