// The split-staged tiles (bf16x6, f16x3) of conv_igemm.h and their tile choice.  Included by conv_split_bf16x6.hip and conv_split_f16x3.hip only:
// each instantiates one precision's kernels.
#pragma once
#include "conv_igemm.h"

namespace stemseg {

// Split-staged tiles (BFV 2 = bf16x6, 3 = f16x3).  3x3x3: eight waves share one weight slab (86 KB in bf16x6, 57 KB in f16x3; one
// workgroup per CU, two waves per SIMD); 2-D and 1x1 tiles keep four-wave shapes (two workgroups per CU) except the big ones
template <int BFV>
struct SplitTiles {
    // 1x3x3 chunks: f16x3 takes 16 channels -- a k-group is then ONE tap x 16 channels and the nine taps fill nine groups exactly; with 8
    // channels a group is two taps x 8 channels and the ninth tap drags a zero tap along: 10 % of the class's MFMAs multiplied zeros
    // (the chip is power-bound under these streams, so MFMAs not issued are time).  bf16x6's three planes of 16 channels do not fit the LDS.
    static constexpr int CK2 = split_chunk_channels(9, BFV);
    using Y3Big = ConvCfg<3, 3, 3, 4, 4, 2, 1, 8, 1, false, BFV>;   // 128 co x (16 rows x 32 cols), 512 threads
    using Y3Med = ConvCfg<3, 3, 3, 4, 2, 2, 2, 4, 1, false, BFV>;   // 128 co x ( 8 rows x 32 cols), 512 threads
    using Y3Small = ConvCfg<3, 3, 3, 4, 2, 1, 2, 4, 1, false, BFV>; // 128 co x ( 4 rows x 32 cols), 512 threads
    using Y2Big = ConvCfg<1, 3, 3, CK2, 4, 2, 1, 8, 1, false, BFV>;   // 128 co x (16 rows x 32 cols), 512 threads (the weight prefetch of a four-wave tile spills)
    using Y2Med = ConvCfg<1, 3, 3, CK2, 2, 2, 2, 2, 1, false, BFV>;   // 128 co x (4 rows x 32 cols)
    using Y2Small = ConvCfg<1, 3, 3, CK2, 2, 1, 2, 2, 1, false, BFV>; // 128 co x (2 rows x 32 cols)
    using Y2M64 = ConvCfg<1, 3, 3, CK2, 2, 2, 1, 4, 1, false, BFV>;   //  64 co x (8 rows x 32 cols)
    using Y1Big = ConvCfg<1, 1, 1, 32, 4, 2, 1, 4, 8, false, BFV>;  // 128 co x 256 voxels
    using Y1Small = ConvCfg<1, 1, 1, 32, 2, 2, 2, 2, 4, false, BFV>; // 128 co x 128 voxels
    using Y1M64 = ConvCfg<1, 1, 1, 32, 2, 2, 1, 4, 8, false, BFV>;  //  64 co x 256 voxels
    using Y1Wide = ConvCfg<1, 1, 1, 32, 4, 2, 2, 4, 8, false, BFV>; // 256 co x 256 voxels, 512 threads: an input element is split once per 256 output channels
    // flat (ragged-width) form of the big 2-D tile: 128 co x 512 flat positions of the whole [T][H + 2][pitch] run (across the
    // frames); PMAX = largest row pitch served (the staged run is tile + 2 PMAX + 8 words)
    template <int PMAX> using Y2Flat = ConvCfg<1, 3, 3, CK2, 4, 2, 1, 8, 16, false, BFV, false, PMAX>;
    // 1x4x4 taps on 16-channel chunks (16 k-groups of one tap x 16 channels): the 7x7 stride-2 stem as a stride-1 4x4 convolution over the
    // space-to-depth image (encoder.hip); 64 co x (16 rows x 32 cols), 512 threads
    using Y4Stem = ConvCfg<1, 4, 4, 16, 2, 2, 1, 8, 1, false, BFV>;
    // block tiles (ConvCfg::BLK): 128 co x (20 rows x 24 columns) as 5 x 3 column blocks of 4 rows x 8 columns, 512 threads -- no junk position on
    // 120 x 216 maps (30 x 27 blocks), where the 16 x 32 tiles compute 128 x 224
    using Y3Blk = ConvCfg<3, 3, 3, 4, 4, 2, 1, 8, 3, false, BFV, false, 0, false, 5>;
    using Y2Blk = ConvCfg<1, 3, 3, CK2, 4, 2, 1, 8, 3, false, BFV, false, 0, false, 5>;
    // the medium 3x3x3 tile's block form: 128 co x (4 rows x 56 columns) as 1 x 7 column blocks (the wave pair that would own the eighth block runs
    // one) -- the decoders' 60 x 108 and 30 x 54 maps compute 60 x 112 / 32 x 56 positions instead of the 8-row x 32-column tile's 64 x 128 / 32 x 64
    // (21 % junk -> 3.6 % / 9.6 %): under the power limit MFMAs not issued are time even where the round count stays (DESIGN.md sections 5f, 5h)
    using Y3Blk7 = ConvCfg<3, 3, 3, 4, 2, 2, 2, 4, 7, false, BFV, false, 0, false, 1>;
    // Measured in round 5 and not kept (profiles/r05b_conv_sweep_f16x3_T32.txt, tile_cfg 6 / 7 / 8 of that build): four-wave halves of the
    // eight-wave tiles, two per CU so that one's staging phases run under the other's MFMA stream -- block_4x 1 076 vs 1 006 us, layer-3 3x3
    // 214 vs 203, 1024 -> 256 110 vs 107, 256 -> 1024 + residual 170 vs 154; and 64-channel chunks for the 1x1 tiles (half the chunk
    // boundaries) -- 1024 -> 256 106 vs 107 (256-co tile), 134 vs 125 (128-co tile), 256 -> 1024 190 vs 154.  Neither barrier overlap
    // nor chunk length is what these kernels wait for.  Likewise the input tile fetched TWO chunks ahead through a second register set
    // (profiles/r05h_sweep{,_ina}.txt): the 128 x 128 tile drops from three to two waves per SIMD (174 VGPRs) and loses 18 % (256 -> 1024
    // 182 vs 154 us), the eight-wave 256 x 256 tile is unchanged (111 vs 108): the step 96.4 vs 98.6 clips/s.  Removed.
    // And PING-PONG forms of the eight-wave tiles (two LDS buffers; waves 0-3 run the MFMA stream of chunk i while waves 4-7 -- their SIMD
    // partners -- split their share of chunk i + 1 into the other buffer, roles swapped at every barrier; B fragments a k-group ahead):
    // bit-identical results, and the same times -- 3x3 tiles within +-1 % (fpn_layer1 2 790 vs 2 796 us, layer-3 3x3 246 vs 239), the 256-co
    // 1x1 tile 5-9 % ahead on the long-K reductions (1024 -> 256 112 vs 119 us) = 0.7 % of the step; the 3x3x3 tile does not fit twice into
    // 160 KB (profiles/r05i_pingpong_tiles.txt).  Why no schedule moves these kernels (profiles/r05i_dvfs_zero_inputs.txt): the SAME launches
    // on all-zero activations -- same instructions, less switching -- run 20-25 % faster (block_4x 995 -> 832 us = 441 TF-eq, fpn_layer1
    // 2 790 -> 2 247): on real data the chip sits at its POWER limit (1.9-2.0 GHz effective under these MFMA streams, GRBM_GUI_ACTIVE / time),
    // and cycles saved by a better schedule come back as a lower clock.  What is left to win is work not done: MFMAs on tap padding (10 tap
    // slots for 9 taps in the 1x3x3 class), junk positions of ragged maps, re-split inputs.
};

// The deep 3x3x3 tile (ConvCfg::DEEP; f16x3 only): 128 co x (8 planes x 8 rows x 8 columns), 512 threads -- wave wn owns output plane wn, its two column
// blocks are the two 4-row x 8-column blocks of the 8 x 8 patch.  Y3Blk stages the planes t - 1, t, t + 1 of a 22 x 26 halo tile per output plane:
// 3 x 22 x 7 = 462 sixteen-byte pieces per chunk and channel for 480 outputs (423 after the zero-halo skip), every input plane fetched, split
// and written to LDS by the workgroups of three output planes.  Here a plane is staged once: 8 x 10 x 3 = 240 pieces for 512 outputs, no zero
// halo plane is ever fetched, all 16 column-block slots are live, and 120 x 216 maps take 405 workgroups per clip instead of 432.  The k order of
// every accumulator is Y3Blk's, so the convolution's output is bit-identical; the GroupNorm partial sums are one slot per workgroup (eight planes),
// i.e. another summation order.  Exists only under the zero-temporal-halo promise with T == 8, and is taken only when the caller asks for it
// (tile_cfg STEMSEG_TILE_CFG_DEEP): it lives outside SplitTiles so that no existing plan can reach it.
struct DeepTiles {
    using Y3Deep = ConvCfg<3, 3, 3, 4, 4, 2, 1, 8, 1, false, 3, false, 0, false, -1>;
};
// the request is honoured where the tile exists: the promise, eight planes (also on the planning shape), a map of whole 8 x 8 patches, 16-byte staging, an
// fp32 output, and a plan that does not split K; everything else plans exactly what it plans without the request
template <class Deep>
static bool deep_tile_eligible(const ConvKParams& p, const ConvKParams& d, const LaunchCtx& L, bool k3) {
    if (!L.deep_tile || !k3 || !p.zero_t_halo || p.T != Deep::TD || d.T != Deep::TD || p.H % Deep::ROWS != 0 || p.W % Deep::TW != 0 || !p.vec4 || p.out_p16 || p.dec_W > 0) return false;
    ConvKParams q = p;
    q.T_all = q.T;
    return plan_ksplit<Deep>(q, L, 0, (int)ceil_div(p.Cin, Deep::CK)) == 1;
}

// split-staged precisions: the weights were packed with stemseg_hip_pack_conv_weight_prec(..., precision).  Tile = the largest whose
// PLANNED launch (with split-K where scratch is given) still covers the chip; tile_cfg 1 / 2 / 3 force big / medium / small, 5 the
// flat form of the big 2-D tile (f16x3; tests and sweeps).  p: the launch, d: its planning shape.
template <int BFV>
int launch_split_family(ConvKParams& p, const ConvKParams& d, const LaunchCtx& L, int tile_cfg, bool k3, bool k2) {
    float* const scratch = L.scratch;
    typedef SplitTiles<BFV> F;
    using Y3Big = typename F::Y3Big; using Y3Med = typename F::Y3Med; using Y3Small = typename F::Y3Small;
    using Y2Big = typename F::Y2Big; using Y2Med = typename F::Y2Med; using Y2Small = typename F::Y2Small; using Y2M64 = typename F::Y2M64;
    using Y1Small = typename F::Y1Small; using Y1Big = typename F::Y1Big; using Y1M64 = typename F::Y1M64; using Y1Wide = typename F::Y1Wide;
    const bool auto_cfg = tile_cfg <= 0 || tile_cfg > 3;
    int cfg = (auto_cfg || tile_cfg == 6) ? 0 : tile_cfg;
    if constexpr (BFV == 3) {
        // Flat tiles (f16x3: the default mode): a 2-D tile of 16 rows x 32 columns computes 128 x 224 positions for a 120 x 216 map and
        // 32 x 64 for layer 3's 30 x 54: 13-21 % of the MFMAs feed positions that are never stored; the flat tile computes the halo
        // columns instead (2 of 56).  Measured (tools/conv_sweep.py, T = 32): a flat workgroup is 6 % slower than a 2-D one at pitch
        // 56 -- by-element epilogue -- and 15-25 % slower at pitch 112 / 224, where the staged run is 1.15x / 1.49x the 2-D tile's
        // piece: the 13-21 % fewer workgroups only pay at pitch <= 56 (layer-3 3x3: 256 -> 224 workgroups, 207 -> 191 us).
        const bool flat_ok = p.vec4 && p.dec_W == 0 && p.in_ys % 4 == 0 && p.W + 2 <= p.in_ys && p.in_ys <= 224 && p.Cout % 128 == 0;
        if (flat_ok && k2 && !p.gn_part && p.in_ts == (int64_t)p.in_H * p.in_ys && p.in_H == p.H + 2 &&
            (tile_cfg == 5 || (auto_cfg && tile_workgroups<Y2Big>(d) >= (scratch ? 96 : 384)))) {
            const double e2d = tile_efficiency<Y2Big>(p.H, p.W);
            const double efl = (double)d.T * p.H * p.W / (512.0 * ceil_div((int64_t)d.T * p.in_ts, 512));
            if (tile_cfg == 5 || (efl > 1.04 * e2d && p.in_ys <= 56)) {
                p.flat_t = 1;
                if (p.in_ys <= 56) return launch_cfg<typename F::template Y2Flat<56>>(p, L);
                if (p.in_ys <= 112) return launch_cfg<typename F::template Y2Flat<112>>(p, L);
                return launch_cfg<typename F::template Y2Flat<224>>(p, L);
            }
        }
    }
    // Block tiles (f16x3): where the big 16 x 32 tile would be chosen and the map wastes > 6 % more of it than of 20 x 24 tiles of 4 x 8 blocks
    // (120 x 216: 10.6 % vs 0), take those; tile_cfg 6 forces them.  Same k order per output: bit-identical to the 16 x 32 tiles.
    if constexpr (BFV == 3) {
        if (deep_tile_eligible<DeepTiles::Y3Deep>(p, d, L, k3)) return launch_cfg<DeepTiles::Y3Deep>(p, L);
    }
    static_assert(F::Y2Blk::ROWS == F::Y3Blk::ROWS && F::Y2Blk::TW == F::Y3Blk::TW && Y2Big::ROWS == Y3Big::ROWS && Y2Big::TW == Y3Big::TW, "blk_gain: the 2-D and 3-D tiles cover the same positions");
    auto blk_gain = [&]() { return tile_efficiency<typename F::Y3Blk>(p.H, p.W) > 1.06 * tile_efficiency<Y3Big>(p.H, p.W); };   // (Y2Blk / Y2Big: the same 20 x 24 / 16 x 32 positions)
    if constexpr (BFV == 3) {
        if (k3 && p.vec4 && (tile_cfg == 6 || (auto_cfg && tile_workgroups<Y3Big>(d) >= 384 && tile_workgroups<typename F::Y3Blk>(d) >= 384 && blk_gain())))
            return launch_cfg<typename F::Y3Blk>(p, L);
        if (k2 && p.vec4 && p.Cout > 64 && (tile_cfg == 6 || (auto_cfg && tile_workgroups<Y2Big>(d) >= (scratch ? 96 : 384) && tile_workgroups<typename F::Y2Blk>(d) >= 384 && blk_gain())))
            return launch_cfg<typename F::Y2Blk>(p, L);
    }
    if (k3) {
        if (cfg == 0) cfg = tile_workgroups<Y3Big>(d) >= 384 ? 1 : (tile_workgroups<Y3Med>(d) >= (scratch ? 32 : 256) ? 2 : 3);
        if constexpr (BFV == 3) {
            // where the medium tile is the choice and the map wastes > 6 % more of it than of 4-row x 56-column block tiles, take those (tile_cfg 7
            // forces them).  Same k order per output: bit-identical to the 8 x 32 tile.
            const double e_b7 = tile_efficiency<typename F::Y3Blk7>(p.H, p.W), e_med = tile_efficiency<Y3Med>(p.H, p.W);
            if (p.vec4 && (tile_cfg == 7 || (auto_cfg && cfg == 2 && e_b7 > 1.06 * e_med)))
                return launch_cfg<typename F::Y3Blk7>(p, L);
        }
        if (cfg == 1) return launch_cfg<Y3Big>(p, L);
        if (cfg == 2) return launch_cfg<Y3Med>(p, L);
        return launch_cfg<Y3Small>(p, L);
    }
    if (k2) {
        if (p.Cout <= 64) return launch_cfg<Y2M64>(p, L);
        if (cfg == 0) {
            const int64_t need = scratch ? 96 : 384;
            cfg = tile_workgroups<Y2Big>(d) >= need ? 1 : (tile_workgroups<Y2Med>(d) >= need ? 2 : 3);
        }
        if (cfg == 1) return launch_cfg<Y2Big>(p, L);
        if (cfg == 2) return launch_cfg<Y2Med>(p, L);
        return launch_cfg<Y2Small>(p, L);
    }
    if (p.Cout <= 64) return launch_cfg<Y1M64>(p, L);
    if (tile_cfg == 3 && p.Cout % 256 == 0) return launch_cfg<Y1Wide>(p, L);
    // reductions / square 1x1 convs onto >= 256 channels: the 256-channel tile splits every input element once per 256 outputs
    // (measured, tools/conv_sweep.py: 1024 -> 256 173 -> 155 us, 256 -> 256 at 4x 806 -> 728 us; short-K expansions lose with it)
    if (auto_cfg && p.Cout % 256 == 0 && p.Cin >= p.Cout && !p.res && tile_workgroups<Y1Wide>(d) >= 128)
        return launch_cfg<Y1Wide>(p, L.without_scratch());
    if (cfg == 0 || cfg > 2) {
        if (BFV == 3) {
            // f16x3 with the one-phase weight schedule (WMODE 1): the 128-voxel tile wins on every 1x1 shape of the step (tools/conv_sweep.py,
            // T = 32: 64 -> 256 444 -> 403 us, 128 -> 512 263 -> 236, 512 -> 2048 128 -> 115, 512 -> 128 146 -> 133, 2048 -> 512 123 -> 115)
            cfg = 2;
        } else {
            cfg = (tile_workgroups<Y1Big>(d) >= (scratch ? 96 : 512)) ? 1 : 2;
            if (p.Cin <= 256 && p.Cout >= 4 * p.Cin && tile_workgroups<Y1Big>(d) < 2048) cfg = 2;
        }
    }
    if (cfg == 1) return launch_cfg<Y1Big>(p, L);
    return launch_cfg<Y1Small>(p, L);
}

}  // namespace stemseg
