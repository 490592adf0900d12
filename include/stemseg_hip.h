/*
 * stemseg_hip.h -- C-ABI of libstemseg_hip.so: the MI355X (gfx950) implementation of STEm-Seg's
 * embed+cluster hot path.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * The reference (sabarim/STEm-Seg) has no FFI of its own: its extension surface is Python
 * (registries + nn.Module / callable contracts).  Each entry point below
 * names the reference interface it stands in for (file:line relative to the reference tree); the
 * Python host-side mirror in stem-seg_amd/stemseg_amd/ binds these with ctypes and re-exposes the
 * reference's class / function names.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success or a negative STEMSEG_E_* code; nothing throws;
 *     stemseg_hip_last_error() gives a thread-local message valid until the next call on the thread.
 *   - no allocation and no ownership transfer: all device memory (inputs, outputs, workspaces) is
 *     provided by the caller; pointers are device pointers unless the name ends in _host.
 *   - work is enqueued on the hipStream_t passed as `void* stream` (NULL = default stream); the
 *     only functions that synchronise with the host are the *_read_* ones, and they say so.
 *   - all floating point is IEEE fp32 (the reference asserts fp32, inference/clusterers.py:12),
 *     labels are int64, masks are uint8.
 */
#ifndef STEMSEG_HIP_H
#define STEMSEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STEMSEG_HIP_ABI_VERSION 11

#define STEMSEG_OK              0
#define STEMSEG_E_INVALID      -1   /* bad argument / unsupported shape               */
#define STEMSEG_E_HIP          -2   /* a HIP runtime call failed (see last_error)     */
#define STEMSEG_E_WORKSPACE    -3   /* workspace too small                            */
#define STEMSEG_E_UNSUPPORTED  -4

#define STEMSEG_MAX_HEAD_OUT   10   /* fused heads kernel: embedding + variance + seediness channels (xytff + seediness = 9) */
#define STEMSEG_MAX_WIDE_HEAD_OUT 64   /* widest linear head of stemseg_hip_wide_level_head / stemseg_hip_wide_heads_backward (two 32-row MFMA blocks) */
#define STEMSEG_MAX_INSTANCES  64   /* upper bound for ClusterParams.max_instances    */
#define STEMSEG_MAX_EMB_DIMS    8
#define STEMSEG_MAX_SEMSEG_CLASSES 128   /* class channels of the semseg loss (YouTube-VIS: 41); target ids are uint8 */

int         stemseg_hip_version(void);
const char* stemseg_hip_last_error(void);
/* number of HIP devices visible, or a negative error (used to fail loudly when there is no GPU) */
int         stemseg_hip_device_count(void);

/* Optional in-library profiler (measurement only): when enabled, every convolution launch is bracketed by a
 * hipEvent pair on its own stream.  profile_read SYNCHRONISES the device, then writes per tag t
 * out_host[3t] = summed kernel ms, out_host[3t+1] = summed algorithmic FLOPs, out_host[3t+2] = launches, and clears the
 * log.  Tags: 8 / 4 / 2 = 3x3x3 conv with an 8 / 4 / 2-row tile, 18 / 14 = 1x1x1 conv (256 / 128-voxel tile), 51 = grouped 3x3 conv,
 * 53 = weight gradient of the 3x3x3 conv (both launches). */
int stemseg_hip_profile_enable(int32_t on);
int stemseg_hip_profile_read(double* out_host, int32_t n_tags);

/* ------------------------------------------------------------------------------------------------
 * Volumes.  A volume is a [C][T][H][W] fp32 tensor addressed as
 *     ptr + c*c_stride + t*t_stride + y*y_stride + x            (strides in floats, x contiguous)
 * which covers the reference's dense NCDHW tensors (N = 1), channel slices of concat buffers and the
 * zero-haloed ("padded") layout the 3x3x3 convolution consumes.  limit = number of floats that may
 * be read starting at ptr (tile over-reads beyond a row are clamped against it).
 * ---------------------------------------------------------------------------------------------- */
typedef struct StemsegVolume {
    float*  ptr;
    int64_t c_stride, t_stride, y_stride;
    int32_t C, T, H, W;
    int64_t limit;
} StemsegVolume;

/* Geometry of the zero-haloed layout for a logical [C][T][H][W] volume: one zero voxel on every side
 * of T, H, W, row pitch rounded up to 4 floats.  out[0..4] = {row_pitch, t_stride, c_stride,
 * total_floats (incl. tail slack), interior_offset}: element (c,t,y,x) lives at
 * base + interior_offset + c*c_stride + t*t_stride + y*row_pitch + x. */
int stemseg_hip_padded_geometry(int32_t C, int32_t T, int32_t H, int32_t W, int64_t out[5]);

/* ------------------------------------------------------------------------------------------------
 * Decoder building blocks (each is also used on its own by the parity tests).
 * Reference: nn.Conv3d / nn.GroupNorm / nn.ReLU / nn.AvgPool3d / F.interpolate as instantiated in
 * stemseg/modeling/embedding_decoder.py:20-96 and common.py:69-78.
 * ---------------------------------------------------------------------------------------------- */

/* Repack a reference-layout conv weight [Cout][Cin][taps] (taps = kt*kh*kw, row-major over kt,kh,kw)
 * into the MFMA implicit-GEMM layout [Cin/4][taps][4][Cout].  Cin % 4 == 0, Cout % 32 == 0. */
int stemseg_hip_pack_conv_weight(const float* w, float* packed, int32_t Cout, int32_t Cin, int32_t taps, void* stream);

/* out[co,t,y,x] = bias[co] + sum_{ci,dt,dy,dx} W[co,ci,dt,dy,dx] * in[ci, t+dt, y+dy, x+dx]
 * "valid" cross-correlation: `in` is the haloed volume (in->T = out->T + kt-1, likewise H, W), so
 * Conv3d(k=3, padding=1) of embedding_decoder.py:21 is `in` = zero-haloed layout.  (kt,kh,kw) is
 * (3,3,3) or (1,1,1).  bias may be NULL.  tile_cfg: 0 = auto, 1..3 = force a tile shape (tuning);
 * STEMSEG_TILE_CFG_DEEP = auto, and where a 3x3x3 f16x3 launch carries the zero-temporal-halo promise
 * (stemseg_hip_conv3d_zero_t_halo), has out->T == 8, out->H % 8 == 0, out->W % 8 == 0, 16-byte aligned input rows and an un-split
 * plan, the DEEP tile: one workgroup owns all eight planes of an 8 x 8 patch and stages every input plane once instead of three
 * times.  The convolution's output is bit-identical to tile_cfg 0's; GroupNorm statistics taken in the epilogue sum their partial
 * sums in another order.  Any other launch plans exactly what tile_cfg 0 plans (StemsegConvPlanRecord.deep tells which it was).
 * splitk_scratch (may be NULL): device scratch of splitk_scratch_floats floats; when a layer yields too few
 * workgroups to fill the chip the input channels are split over up to 16 workgroups per tile, partial sums go to the
 * scratch (k * Cout*T*H*W floats) and a second kernel reduces them in fixed order (+ bias) into `out`. */
#define STEMSEG_TILE_CFG_DEEP 8
typedef struct StemsegConvEpilogue {
    int32_t      relu;             /* max(v, 0) last                                                                     */
    const float* residual;         /* NULL or a tensor added before the ReLU, addressed at the OUTPUT's (c,t,y,x) with: */
    int64_t      res_c_stride, res_t_stride, res_y_stride;
    int32_t      decode_H, decode_W; /* > 0: the 1x1x1 conv runs on a flat [C][V] input (in->T = in->H = 1, in->W = V) and
                                        voxel v is stored at (t,y,x) = (v/(H*W), (v/W)%H, v%W) of `out` (e.g. dense -> haloed) */
    int32_t      precision;        /* arithmetic of the matrix products; packed_w must be packed for the same mode.
                                      STEMSEG_PRECISION_F32: v_mfma_f32_32x32x2_f32 on the fp32 operands (exact products);
                                      packed_w from stemseg_hip_pack_conv_weight.
                                      STEMSEG_PRECISION_BF16X6: every fp32 operand is split EXACTLY into three bf16 terms
                                      (hi + mid + lo, 24 significand bits) and a*b is the sum of the six products of weight
                                      >= 2^-16 on the bf16 matrix cores, fp32 accumulation: the dropped products are <= 2^-23
                                      |a*b|, below the rounding of the fp32 accumulation itself -- fp32-level results, fp32's
                                      exponent range, 2.7x the fp32-MFMA rate.
                                      STEMSEG_PRECISION_F16X3: both operands are scaled by a power of two (activations by 2^-2,
                                      every OUTPUT CHANNEL's weights so that its largest lands in [2^13, 2^14)) and split into two fp16
                                      terms (hi + lo: 22 significand bits, fp32 has 24); the low activation term is stored as
                                      lo * 2^11 and meets a third weight operand, hi_w * 2^-11, so hi is a normal fp16 number and
                                      the pair keeps 22 bits (or 2^-36 absolute) for 2.5e-4 <= |a| < 2.6e5.  a*b = lo_w*hi_a +
                                      hi_w*lo_a + hi_w*hi_a on the fp16 matrix cores, fp32 accumulation, accumulators scaled back
                                      exactly: the dropped lo*lo product and the split remainder are <= 2^-22 |a*b| -- measured
                                      below the rounding spread of fp32 accumulation orders -- at HALF the matrix work of
                                      bf16x6.  |a| >= 2.6e5 overflows (inf in, non-finite out: see stemseg_hip_nonfinite_flags).
                                      packed_w of both split modes from stemseg_hip_pack_conv_weight_prec. */
    /* Planning shape: the launch holds `frames` frames (its T axis, or -- flat [C][V] input -- V / the per-frame voxel count), and
       the tile shape and split-K factor are decided as if it held `plan_frames`, counting on `plan_scratch_floats` of split-K
       scratch (the real scratch must hold frames / plan_frames times what the plan uses, or the call fails).  The K-partition of a
       split-K launch is a summation order: decided this way, every output bit is a function of the per-frame layer shape, the
       precision and plan_frames -- not of how many frames share the launch.  plan_frames = 0: decide on the real shape. */
    int32_t      frames, plan_frames;
    int64_t      plan_scratch_floats;
} StemsegConvEpilogue;
#define STEMSEG_PRECISION_F32    0
#define STEMSEG_PRECISION_BF16X6 2      /* (1 was the two-term bf16 split of rounds 2-4: ~1e-4 on the maps, retired) */
#define STEMSEG_PRECISION_F16X3  3
/* Split-staged packings, by precision code.  2: per channel chunk [k-group][hi | mid | lo][lane half][Cout] x 8 bf16; 3: the same
 * order with two fp16 planes (hi, lo) of the scaled weights + per output channel a float 1 / (weight scale x activation scale) and
 * the bits of max|w| of the channel (8 * Cout bytes).  bytes = 0 for any other code. */
int64_t stemseg_hip_packed_weight_bytes_prec(int32_t Cout, int32_t Cin, int32_t taps, int32_t precision);
int stemseg_hip_pack_conv_weight_prec(const float* w, void* packed, int32_t Cout, int32_t Cin, int32_t taps, int32_t precision, void* stream);
/* (kt,kh,kw) additionally accepts (1,3,3): a 2-D 3x3 convolution over every t-plane (the encoder's frames).
 * epilogue may be NULL (plain conv + bias). */
int stemseg_hip_conv3d(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                       int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch,
                       int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue, void* stream);
/* stemseg_hip_conv3d with a PROMISE: the temporal halo planes of `in` -- plane 0 and plane in->T - 1 = out->T + 1, every channel,
 * all rows and columns -- hold zeros, as in the zero-haloed feature buffers that make the convolution a padding = 1 one.  The
 * split-staged precisions (bf16x6, f16x3) then leave out, in the workgroups of the first and of the last output plane, the k-groups
 * whose taps all fall into the zero plane (2 of 7 per channel chunk), their weights and the plane's fetch and operand split; every
 * other product is formed and summed in the same order, so the output equals stemseg_hip_conv3d's on the same input (the sign of an
 * exact zero aside).  out->T == 1 and the fp32-input precision run exactly as stemseg_hip_conv3d.  kt must be 3 (an argument error
 * otherwise).  The result is UNSPECIFIED if plane 0 or plane out->T + 1 of `in` is not all zero: stemseg_hip_conv3d is the valid
 * cross-correlation over whatever the view holds.  The decoders (stemseg_hip_decoder_forward) make this promise for all seven of
 * their 3x3x3 stages: their workspace buffers are zeroed by stemseg_hip_decoder_init_workspace and only interiors are written, and
 * features passed with input_layout == 2 ("already zero-haloed") carry it as part of that layout.
 * stats != NULL: additionally the GroupNorm statistics of the output over `groups` channel groups, with the arguments, restrictions
 * and results of stemseg_hip_conv3d_gn (gn_scratch as there; plain bias epilogue).  stats == NULL: groups, eps, gn_scratch unused.
 * Additive: joined ABI 11 without changing any earlier entry point, so STEMSEG_HIP_ABI_VERSION stays 11. */
int stemseg_hip_conv3d_zero_t_halo(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                   int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch,
                                   int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue, int32_t groups, float eps,
                                   float* stats, double* gn_scratch, void* stream);
/* ... as ONE STAGE of a decoder whose descriptor carries `plan_clips` runs it: the split-K factor is planned for that many clips
 * (StemsegDecoderDesc.plan_clips; 0 / 1: stemseg_hip_conv3d_zero_t_halo).  With the scratch size the decoder gives the stage's branch, the
 * output has the bits stemseg_hip_decoder_forward computes for it.  Additive. */
int stemseg_hip_conv3d_zero_t_halo_clips(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                         int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch,
                                         int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue, int32_t groups, float eps,
                                         float* stats, double* gn_scratch, int32_t plan_clips, void* stream);

/* ... on a CLIP BATCH, as a decoder stage of n_clips clips launches it (the clip is a grid dimension of the one launch): clip c's input and
 * output volumes lie c * in_clip_stride / c * out_clip_stride floats (multiples of 4) behind `in` / `out`.  No split-K scratch, no
 * statistics, no residual.  Every launch decision is taken on one clip, so a clip's output is what the single-clip call gives.  Additive. */
int stemseg_hip_conv3d_zero_t_halo_batch(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                         int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, const StemsegConvEpilogue* epilogue,
                                         int32_t n_clips, int64_t in_clip_stride, int64_t out_clip_stride, void* stream);

/* DRY RUN of the launch decision of stemseg_hip_conv3d / _conv3d_gn / _conv3d_zero_t_halo: the same dispatch code runs up to the point
 * where it would launch, appends one record per kernel launch it would make (a planned row cut makes two) and makes NO HIP call -- it
 * needs no device.  Pointers (in->ptr, out->ptr, bias, splitk_scratch, epilogue->residual) are used for their nullness and alignment
 * only and are never dereferenced, so made-up addresses serve.  Arguments as stemseg_hip_conv3d without the weights; `form`: 0 =
 * stemseg_hip_conv3d, STEMSEG_PLAN_GN = stemseg_hip_conv3d_gn (precision taken from epilogue->precision, the rest of the epilogue unused),
 * STEMSEG_PLAN_ZERO_T_HALO = stemseg_hip_conv3d_zero_t_halo, both = that entry with statistics; gn_groups as `groups` there.
 * records[0 .. min(*count, capacity)) are written, *count = the launches the call would make.  An argument the real call refuses is
 * refused here with the same message.  Additive: joined ABI 11 without changing any earlier entry point. */
typedef struct StemsegConvPlanRecord {
    int32_t kt, kh, kw;            /* taps of the tile                                                                          */
    int32_t ck, mt;                /* input channels per chunk, output channels per workgroup                                    */
    int32_t rows, tw, nt;          /* 2-D tiles: rows x columns; nt = positions per workgroup (flat tiles: the run of the plane) */
    int32_t flat, pmax;            /* flat tile and the largest row pitch it serves                                              */
    int32_t gl, blk;               /* direct-to-LDS staging; block rows of the 4 x 8 block tiles (0: none)                       */
    int32_t threads;
    int32_t precision;             /* STEMSEG_PRECISION_* of the tile                                                            */
    int32_t ksplit, chunks_per_split, nchunks;
    int32_t grid[3];
    int32_t row0, row1;            /* output rows [row0, row1) of the map this launch covers                                     */
    int32_t vec4, vec_epi;         /* 16-byte input staging / 16-byte epilogue, as the kernel is launched                        */
    int32_t reduce;                /* split-K reduce kernel: 0 none, 1 the 16-byte form, 2 the scalar form                       */
    int32_t gn;                    /* GroupNorm statistics: 0 none, 1 per tile in the conv's epilogue, 2 in the split-K reduce,
                                      3 a separate pass over the output                                                          */
    int32_t zero_t_halo;           /* the temporal-halo promise reaches the kernel                                               */
    int32_t nb;
    int32_t deep;                  /* output planes per workgroup of the deep 3x3x3 tile (0: a tile of one plane)                 */
} StemsegConvPlanRecord;
#define STEMSEG_PLAN_GN          1
#define STEMSEG_PLAN_ZERO_T_HALO 2
int stemseg_hip_conv3d_plan(const StemsegVolume* in, const float* bias, const StemsegVolume* out, int32_t kt, int32_t kh, int32_t kw,
                            int32_t tile_cfg, const float* splitk_scratch, int64_t splitk_scratch_floats,
                            const StemsegConvEpilogue* epilogue, int32_t form, int32_t gn_groups, StemsegConvPlanRecord* records,
                            int32_t capacity, int32_t* count);
/* ... with the split-K factor planned for `plan_clips` clips, as a stage of a decoder with StemsegDecoderDesc.plan_clips decides it (0 / 1:
 * stemseg_hip_conv3d_plan).  Additive. */
int stemseg_hip_conv3d_plan_clips(const StemsegVolume* in, const float* bias, const StemsegVolume* out, int32_t kt, int32_t kh, int32_t kw,
                                  int32_t tile_cfg, const float* splitk_scratch, int64_t splitk_scratch_floats,
                                  const StemsegConvEpilogue* epilogue, int32_t form, int32_t gn_groups, int32_t plan_clips,
                                  StemsegConvPlanRecord* records, int32_t capacity, int32_t* count);

/* Grouped 3x3 convolution, padding 1, stride 1 or 2 (the ResNeXt bottleneck conv2, resnet.py:240-249, and the stride-in-3x3 conv2,
 * :227-238), + bias, + ReLU when relu != 0:
 *     out[co,t,y,x] = bias[co] + sum_{ci in group(co), dy, dx} W[co,ci,dy,dx] * in[ci, t, s*y+dy, s*x+dx]
 * `in` is the zero-haloed 2-D view (in->H, in->W = map rows / columns + 2; in->C = Cout), out [Cout][T][(H-1)/s+1][(W-1)/s+1] any
 * strides.  Cout per group == Cin per group, 4, 8, 16, 32 or 64 channels (one group: any multiple of 16); Cout % 16 == 0.  Weights
 * [Cout][Cin/groups][3][3] packed for the precision by stemseg_hip_pack_grouped_conv_weight (bytes: stemseg_hip_packed_grouped_weight_bytes,
 * 0 = unsupported): per 16 output channels a window of max(16, Cin per group) input channels, so groups of 4 / 8 channels issue 4x / 2x
 * their algorithmic MFMA work and wider ones 1x (10/9 in the split modes).  Precision codes and operand arithmetic as
 * StemsegConvEpilogue.precision (f16x3: a non-finite output for |activation| >= 2.6e5; such an activation may also make the other
 * groups of its 16-channel block non-finite).  No split-K and no scratch: every output bit is a function of the per-frame shape and
 * the precision; plan_frames (>= 0) is accepted for symmetry with the other convolutions and changes nothing.  No host sync, no
 * allocation (graph-capture safe). */
int64_t stemseg_hip_packed_grouped_weight_bytes(int32_t Cout, int32_t Cin_g, int32_t groups, int32_t precision);
int stemseg_hip_pack_grouped_conv_weight(const float* w, void* packed, int32_t Cout, int32_t Cin_g, int32_t groups, int32_t precision, void* stream);
int stemseg_hip_conv2d_grouped(const StemsegVolume* in, const void* packed_w, const float* bias, const StemsegVolume* out, int32_t groups,
                               int32_t stride, int32_t relu, int32_t precision, int32_t plan_frames, void* stream);

/* Convolution + the GroupNorm statistics of its output in ONE pass (embedding_decoder.py:21-23: Conv3d followed by
 * GroupNorm): the conv's epilogue -- or, for split-K launches, its reduce kernel -- leaves per-tile fp64 partial sums in
 * gn_scratch (>= stemseg_hip_conv3d_gn_scratch_doubles(Cout, groups) doubles) and one small launch combines them in fixed
 * order (no atomics: bit-identical run to run) into stats[2g] = mean, stats[2g+1] = 1/sqrt(biased_var + eps), so the
 * conv output is not read again for the statistics.  Plain bias epilogue only; groups of 4 or 8 channels take the fused
 * path, any other group size runs stemseg_hip_conv3d + stemseg_hip_groupnorm_stats (dense `out` required then). */
int64_t stemseg_hip_conv3d_gn_scratch_doubles(int32_t Cout, int32_t groups);
int stemseg_hip_conv3d_gn(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                          int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch,
                          int64_t splitk_scratch_floats, int32_t precision, int32_t groups, float eps,
                          float* stats, double* gn_scratch, void* stream);

/* GroupNorm statistics over a dense [C][S] tensor (S = T*H*W), `groups` contiguous channel groups:
 * stats[2g] = mean, stats[2g+1] = 1/sqrt(biased_var + eps).  scratch: >= groups*128 doubles. */
int stemseg_hip_groupnorm_stats(const float* x, int32_t C, int64_t S, int32_t groups, float eps,
                                float* stats, double* scratch, void* stream);

/* y = ReLU(GroupNorm(x)) optionally followed by AvgPool3d(3, stride (2,1,1), padding 1,
 * count_include_pad) -- embedding_decoder.py:22-24.  `x` dense [C][T][H][W]; `out` any volume with
 * out->T == (pool ? (T+1)/2 : T). */
int stemseg_hip_gn_relu_pool(const float* x, int32_t C, int32_t T, int32_t H, int32_t W, int32_t groups,
                             const float* stats, const float* gamma, const float* beta, int32_t pool,
                             const StemsegVolume* out, void* stream);

/* F.interpolate(mode='trilinear', align_corners=False) with integer scale (st, sy, sx) -- common.py:77-78 and
 * online_chainer.py:127-140 (sx = sy = 4, st = 1).  `in` dense [C][T][H][W]; out->T/H/W = scaled dims. */
int stemseg_hip_upsample_trilinear(const float* in, int32_t C, int32_t T, int32_t H, int32_t W,
                                   int32_t st, int32_t sy, int32_t sx, const StemsegVolume* out, void* stream);

/* Copy a dense feature stack into a volume (typically the zero-haloed layout).
 * layout 0: in = [C][T][H][W] (the head input of embedding_decoder.py:101-109);
 * layout 1: in = [T][C][H][W] (what the 2-D encoder emits, model_builder.py:154-169). */
int stemseg_hip_copy_to_volume(const float* in, int32_t layout, const StemsegVolume* out, void* stream);

/* Fused 1x1x1 heads (embedding_decoder.py:131-143, seediness_decoder.py:112, inference_model.py:148):
 * out[o, v] = act_o( bias[o] + sum_c w[o][c] * x[c, v] ),  x dense [Cin][V], out dense [n_out][V].
 * act codes: 0 identity, 1 tanh(0.25*z) + grid, 2 sigmoid, 3 exp(z)*10, 4 identity + grid.
 * grid_axis[o]: 0 none, 1 t, 2 y, 3 x -- the coordinate added for act 1/4 (embedding_utils.py:44-120);
 * grid_t/y/x are the linspace vectors of embedding_utils.py:28-41 (length T, H, W). */
int stemseg_hip_heads(const float* x, int32_t Cin, int32_t T, int32_t H, int32_t W,
                      const float* w, const float* bias, int32_t n_out, const int32_t* act_host,
                      const int32_t* grid_axis_host, const float* grid_t, const float* grid_y, const float* grid_x,
                      float* out, void* stream);

/* Overflow guard: flags[b] = 1 when chunk b (of n_flags equal chunks) of x holds an inf / NaN, else 0; every flag is rewritten by
 * every call (no reset needed, graph-replay safe).  The split convolution modes have a finite operand range (f16x3: |activation| <
 * 2.6e5); beyond it their outputs are non-finite BY CONSTRUCTION and the ReLUs / pools keep NaN, so a non-finite head output is the
 * signal to re-run the clip in STEMSEG_PRECISION_BF16X6 (fp32's range) -- never cluster such maps (ClipPipeline.step_checked). */
int stemseg_hip_nonfinite_flags(const float* x, int64_t n, int32_t* flags, int32_t n_flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole decoder: SqueezingExpandDecoder.forward (embedding_decoder.py:101-145) and the seediness twin
 * (seediness_decoder.py:92-112), optionally with the bandwidth activation of inference_model.py:148.
 * ---------------------------------------------------------------------------------------------- */
typedef struct StemsegDecoderDesc {
    int32_t struct_bytes;        /* = sizeof(StemsegDecoderDesc), checked                                   */
    int32_t in_channels;         /* FPN channels (256)                                                      */
    int32_t inter[4];            /* INTER_CHANNELS for the 32x,16x,8x,4x branches (256,256,128,128)          */
    int32_t T, H4, W4;           /* clip length and 1/4-resolution output size; H4 % 8 == 0, W4 % 8 == 0    */
    int32_t gn_groups;           /* 32; 0 = NORMALIZATION_LAYER 'none' (nn.Identity, model_builder.py:29-33): gn_w / gn_b must then be ones / zeros */
    float   gn_eps;              /* 1e-5                                                                    */
    int32_t pool[3];             /* common.py:8-24 : temporal pooling layer i: 0 absent, 1 AvgPool3d, 2 MaxPool3d (POOL_TYPE; T=8: 1,1,0) */
    int32_t t_scale[3];          /* common.py:27-35: temporal up-sampling factors (T=8: 1,2,2)              */
    int32_t n_out;               /* head output channels: 1..10 = fused heads kernel (emb + var + seed / seediness);
                                    a multiple of 32 = plain linear head through the 1x1x1 MFMA conv (semseg logits,
                                    semseg_decoder.py:116; weights->head_w is then a packed conv weight, act is ignored) */
    int32_t act[STEMSEG_MAX_EMB_DIMS * 2];        /* per output channel, see stemseg_hip_heads          */
    int32_t grid_axis[STEMSEG_MAX_EMB_DIMS * 2];
    int32_t input_layout;        /* 0: [C][T][h][w] dense, 1: [T][C][h][w] dense, 2: already zero-haloed (a promise: every
                                    halo plane, row and column holds zeros -- see stemseg_hip_conv3d_zero_t_halo) */
    int32_t concurrency;         /* 0: every launch on the caller's stream.  k >= 1: the 32x / 16x / 8x branches run
                                    on the library's internal stream set (k-1) % 4 beside the 4x branch (fork / join by
                                    events on the caller's stream; the call is still stream-ordered for the caller).
                                    Decoders that may overlap (embedding + seediness) should use different sets.     */
    int32_t detached;            /* with concurrency >= 1: ALL work (also the 4x branch and the heads) runs on the internal
                                    streams and the call returns without joining; the caller must enqueue
                                    stemseg_hip_decoder_join(concurrency, stream) before it consumes `out` or re-uses the
                                    inputs / workspace.  Lets a twin decoder be enqueued in between (both fill the chip). */
    int32_t precision;           /* STEMSEG_PRECISION_F32 | _BF16X6 | _F16X3 for every convolution of the decoder
                                    (weights in StemsegDecoderWeights must be packed for the same mode)                    */
    int32_t n_clips;             /* clip batch: the decoder runs n_clips clips (0 / 1: one) in ONE launch per stage -- the clip is a grid
                                    dimension of every kernel.  Every launch decision is taken on one clip's shape (and on plan_clips
                                    below, never on n_clips), so a clip's output is bit-identical whatever the batch.  The workspace
                                    holds n_clips clip plans.                                                                    */
    int64_t feat_clip_stride[4]; /* n_clips > 1: floats between consecutive clips' input feature buffers, per level (feats[i] is
                                    clip 0's)                                                                                     */
    int64_t out_clip_stride;     /* n_clips > 1: floats between consecutive clips' outputs (0: n_out * T * H4 * W4, i.e. dense)   */
    /* added after ABI 11; the older size (struct_bytes = offsetof(StemsegDecoderDesc, plan_clips)) is accepted and means 0 */
    int32_t plan_clips;          /* clips the split-K factor of every convolution is PLANNED for (0 / 1: one clip, the plans and bits of
                                    the older descriptor).  A launch splits K until about 1.25 workgroups per CU are planned; counted on one
                                    clip, the small-map stages of a 4-clip call split 2 .. 16 ways although the call fills the chip several
                                    times over, and every split is a set of partial slabs written and read back.  With plan_clips = k the
                                    workgroups of k clips are counted.  It is a constant of the model, NOT the n_clips of the call: the K
                                    partition is a summation order, and with the same plan_clips a clip's output is bit-identical alone and
                                    in any batch.  Tile shapes, row cuts and the workspace layout do not depend on it.  The price: a call of
                                    fewer clips than planned runs its smallest stages on fewer workgroups than it would have split into. */
    /* The reserved word carries ONE switch, for A/B runs.  0 (what every caller has passed so far): the block_4x convolution, the largest launch
       of a decoder, asks for the deep 3x3x3 tile (STEMSEG_TILE_CFG_DEEP: f16x3 and T == 8; anything else runs as before).  1: the automatic tile
       choice, i.e. the launches of the library before the deep tile.  Same convolution output either way; the stage's GroupNorm statistics differ
       in the order of their partial sums.  Any other value is an argument error; the older descriptor size means 1. */
    int32_t reserved;            /* 0 */
} StemsegDecoderDesc;

typedef struct StemsegDecoderWeights {
    /* 3x3x3 convs in order block_32x.{0,4,8}, block_16x.{0,4}, block_8x.0, block_4x.0 (packed layout) */
    const float* conv_w[7];
    const float* conv_b[7];
    const float* gn_w[7];
    const float* gn_b[7];
    const float* fuse_w[3];      /* conv_16, conv_8, conv_4 (1x1x1, no bias), packed layout.  Between the last GroupNorm + ReLU of a branch and the
                                    heads' activations the decoder is LINEAR (up-sampling, concatenation, these convs, the 1x1x1 heads), and a
                                    caller may hand over the product matrices instead of the factors:
                                    * fuse_w[2] = NULL: conv_4 folded into the heads -- head_w = W_heads . W_conv4 over the inter[2] + inter[3]
                                      channels of the last concat buffer (dense [n_out][inter[2] + inter[3]], or the packed 1x1x1 weight with that
                                      Cin for a wide head); the inter[3]-channel map is never materialised;
                                    * fuse_w[0..2] = NULL (n_out <= STEMSEG_MAX_HEAD_OUT): the whole tail folded -- 1x1x1 convs commute with
                                      up-sampling, so heads(x) = up(up(up(M32 x32) + M16 y16) + M8 y8) + M4 y4 and head_w = [M32 | M16 | M8 | M4],
                                      M_l dense [n_out][inter[l]] (M4 = Wh W4b, M8 = Wh W4a W8b, M16 = Wh W4a W8a W16b, M32 = Wh W4a W8a W16a for
                                      W = [Wa | Wb] over the (up-sampled, own) halves of a concat input): every level adds its n_out-channel
                                      share at its own resolution, and the heads normalise the 4x branch's raw conv output as they read it.
                                    Either way the same function, within fp32 round-off of the step-by-step form. */
    const float* head_w;         /* [n_out][inter[3]] row-major */
    const float* head_b;         /* [n_out] (zero where the reference conv has no bias) */
    const float* grid_t;         /* [T], [H4], [W4] linspace vectors (may be NULL if no act uses the grid) */
    const float* grid_y;
    const float* grid_x;
} StemsegDecoderWeights;

size_t stemseg_hip_decoder_workspace_bytes(const StemsegDecoderDesc* desc);
/* zero the halos; call once per (workspace, desc) before the first forward */
int stemseg_hip_decoder_init_workspace(const StemsegDecoderDesc* desc, void* workspace, size_t ws_bytes, void* stream);
/* Debug check (SYNCHRONISES the stream): every slice of the workspace is followed by a 64-word guard block that init_workspace filled
 * with a canary; *n_bad_host = guard words that no longer hold it (an out-of-slice write by some kernel), *first_bad_host = float
 * offset of the first such word in the workspace (-1: none).  Costs one tiny launch + one 16-byte read-back. */
int stemseg_hip_decoder_check_workspace(const StemsegDecoderDesc* desc, const void* workspace, size_t ws_bytes, int32_t* n_bad_host,
                                        int64_t* first_bad_host, void* stream);
/* feats[0..3] = 32x,16x,8x,4x feature stacks in desc->input_layout; out = [n_out][T][H4][W4] dense */
int stemseg_hip_decoder_forward(const StemsegDecoderDesc* desc, const StemsegDecoderWeights* weights,
                                const float* const feats[4], float* out,
                                void* workspace, size_t ws_bytes, void* stream);

/* make `stream` wait for a detached decoder_forward issued with the same concurrency set */
int stemseg_hip_decoder_join(int32_t concurrency, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2-D encoder: ResNet-50/101 + FPN over the T frames of a clip (backbone/resnet.py:105-113, fpn.py:47-69,
 * model_builder.py:154-169).  FrozenBatchNorm (make_layers.py:51-63) is folded into conv weight / bias by the caller.
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_MAX_ENCODER_BLOCKS 40

typedef struct StemsegEncoderDesc {
    int32_t struct_bytes;        /* = sizeof(StemsegEncoderDesc)                                        */
    int32_t blocks[4];           /* bottleneck blocks per stage: R-50 {3,4,6,3}, R-101 {3,4,23,3}       */
    int32_t T, H, W;             /* frames per call and padded frame size (multiples of 32)              */
    int32_t out_channels;        /* 256                                                                  */
    int32_t precision;           /* STEMSEG_PRECISION_F32 | _BF16X6 | _F16X3 (every 3x3 / 1x1 conv; the 7x7 stem is always fp32-input MFMA) */
    int32_t n_clips;             /* >= 1: the T frames are n_clips consecutive clips of T / n_clips frames; each clip's four maps
                                    go to their own output volumes (frames are independent in the encoder, so several clips
                                    share one pass: layer3 / layer4 launches grow from 0.4 to n_clips x 0.4 waves of the chip) */
    int32_t clip_frames;         /* 0: T / n_clips.  > 0 with clip_stride > 0: the clips are OVERLAPPING windows of clip_frames
                                    frames every clip_stride frames of the pass ((n_clips - 1) * clip_stride + clip_frames == T),
                                    the way inference/main.py:23-49 cuts a sequence: a frame shared by two clips goes through
                                    the encoder once (the reference's cross-clip feature cache, inference_model.py:83-108) and
                                    each clip's window of the FPN maps is copied to its output volumes */
    int32_t clip_stride;
    int32_t plan_frames;         /* > 0: every convolution of the pass decides its tile shape and split-K factor as if the pass held
                                    this many frames (StemsegConvEpilogue.plan_frames): a frame's four maps are then bit-identical
                                    whatever T, n_clips and the windowing of the pass are -- one clip, a batch of clips, or the
                                    union of overlapping windows -- which is what makes an N-rank sequence job reproduce the
                                    one-rank labels.  0: decide on the real T (fastest for that T; results depend on it). */
    int32_t fuse_tail;           /* bit (stage - 1) set (1 | 2 | 4 = stages 1-3), f16x3 mode: conv3 (+ bias + identity + ReLU) of a bottleneck block and conv1 (+ bias + ReLU) of
                                    the next one run as ONE back-to-back kernel (resnet.py:262-282 of two consecutive blocks): the 4x-wide block
                                    output is written once and never read back by conv1, and conv2 hands its output over as fp16 operand
                                    planes.  Same operands and k order: bit-identical to the separate launches wherever those run without
                                    split-K.  0: three launches per block everywhere (rounds 1-5).  Bits 3-4 pick stage 3's kernel (A/B):
                                    0 = the library's choice (one wave per SIMD, bit-identical like stages 1-2), 1 (value 8) = the
                                    16-column form (fp32 round-off apart from the separate launches), 2 (value 16) = one wave per SIMD.
                                    Bit 5 (value 32): keep the stand-alone projection-shortcut launches of stages 1-2 (A/B, tests).  Clear
                                    (the default): the fused tail of the first block of stages 1-2 computes the block's projection shortcut
                                    itself from the block's input -- same operands, k order and rounding steps as the launch, the same
                                    bits -- and the shortcut map is neither written nor read.
                                    Bits 6, 7, 8 (values 64, 128, 256): keep the stand-alone end of stage 1 / 2 / 3 -- conv3 of the stage's
                                    last block, the level's FPN lateral 1x1 and the stride-2 sub-sample pass in front of the next stage.
                                    Clear (the default): one stage-end tail computes all three -- the stage output is written once, the
                                    lateral's K loop reads it from registers, the kept quarter goes straight to the next stage's input.
                                    Same operands, k order and rounding steps: the same bits.  It engages where the stage's bit (0-2) is
                                    set, the stage has two blocks or more, the level's dense-lateral add pass applies (w % 4 == 0 ...),
                                    and neither that block's conv2 nor the stand-alone lateral would split K on the planning shape.
                                    The fused tail engages only where conv2_groups == 1 and mid * 4 == 256 << stage (today's widths);
                                    any other block runs its three launches whatever this field says. */
    /* ---- backbone architecture (MODEL.RESNETS, resnet.py:64-89, :227-249).  Fields added after ABI 11 shipped: a descriptor of the
       older size (struct_bytes = offsetof(StemsegEncoderDesc, conv2_groups)) is accepted and means 1, 64, 0.  0 in the first two
       also means the default.  Stage s (0..3) has mid_s = conv2_groups * width_per_group << s bottleneck channels (buffers M1 and M2
       are sized from them) and 256 << s output channels. */
    int32_t conv2_groups;        /* NUM_GROUPS: conv2 (3x3) of every block is a grouped convolution (stemseg_hip_conv2d_grouped);
                                    > 1 requires width_per_group 4 or 8 (4..64 channels per group over the four stages) and mid_0 % 32 == 0 */
    int32_t width_per_group;     /* WIDTH_PER_GROUP; with conv2_groups == 1 it must be 64 */
    int32_t stride_in_3x3;       /* 1 = STRIDE_IN_1X1 False: the first block of stages 2-4 runs conv1 at the previous stage's resolution and
                                    conv2 with stride 2 (grouped kernel, also with one group); the projection shortcut still reads
                                    the 2x-subsampled input.  0 = stride in conv1 (the default network) */
} StemsegEncoderDesc;

typedef struct StemsegEncoderWeights {
    const float* stem_w;         /* [147][64] tap-major ((c*7+dy)*7+dx), BN folded */
    const float* stem_b;         /* [64] */
    const float* stem_w_s2d;     /* optional, f16x3 mode: the stem as a stride-1 4x4 convolution over the space-to-depth image -- weights
                                    [64][12][1][4][4] with W2[co][(p*2+q)*3+c][a][b] = w[co][c][2a+p-1][2b+q-1] (0 where an index is -1),
                                    packed by stemseg_hip_pack_conv_weight_prec(taps = 16, STEMSEG_PRECISION_F16X3).  NULL: the exact
                                    fp32-MFMA stem from stem_w in every mode */
    /* per bottleneck block, in network order; conv weights in the packed layout of stemseg_hip_pack_conv_weight (_prec for the split
       modes).  conv2_w[i] holds the packing of stemseg_hip_pack_grouped_conv_weight instead wherever conv2 runs on the grouped kernel:
       every block when conv2_groups > 1, and with stride_in_3x3 the first block of stages 2-4 */
    const float* conv1_w[STEMSEG_MAX_ENCODER_BLOCKS];   const float* conv1_b[STEMSEG_MAX_ENCODER_BLOCKS];
    const float* conv2_w[STEMSEG_MAX_ENCODER_BLOCKS];   const float* conv2_b[STEMSEG_MAX_ENCODER_BLOCKS];
    const float* conv3_w[STEMSEG_MAX_ENCODER_BLOCKS];   const float* conv3_b[STEMSEG_MAX_ENCODER_BLOCKS];
    const float* down_w[STEMSEG_MAX_ENCODER_BLOCKS];    const float* down_b[STEMSEG_MAX_ENCODER_BLOCKS];   /* first block of a stage only */
    const float* fpn_inner_w[4]; const float* fpn_inner_b[4];     /* fpn_inner1..4 (levels 4x, 8x, 16x, 32x) */
    const float* fpn_layer_w[4]; const float* fpn_layer_b[4];
} StemsegEncoderWeights;

size_t stemseg_hip_encoder_workspace_bytes(const StemsegEncoderDesc* desc);
/* Debugging aid: float offsets of the encoder plan's buffers inside the workspace (S0, X1, A, B, Cst[4], M1[4], M2, DS, XS, L[4], FO[4],
 * SK, total: 25 values, -1 = absent). */
int stemseg_hip_encoder_plan_offsets(const StemsegEncoderDesc* desc, int64_t* out25);
/* Debugging aid: bit k of *mask_out = the last block of stage k + 1 ends in the stage-end tail (fuse_tail bits 6-8), as far as the descriptor
 * decides; the pass then takes it where that block's conv2 runs un-split on the planning shape.  Additive: STEMSEG_HIP_ABI_VERSION stays 11. */
int stemseg_hip_encoder_stage_end_mask(const StemsegEncoderDesc* desc, int32_t* mask_out);

/* The stem alone (resnet.py:285-304 up to the ReLU; FrozenBN folded into w / bias): frames float32 [T][3][H][W] ->
 * out float32 [64][T][H/2][W/2] = relu(conv7x7 stride 2 pad 3 + bias).  w_tap_major: [3*7*7][64] (tap-major: the folded
 * [64][3][7][7] weight reshaped to [64][147] and transposed).  What stemseg_hip_encoder_forward runs first; exported for tests
 * and for the co-residency probe (tools/stem_corun_probe.py). */
int stemseg_hip_stem_conv(const float* frames, const float* w_tap_major, const float* bias, float* out, int32_t T, int32_t H, int32_t W,
                          void* stream);
/* The encoder's streaming passes on their own (csrc/encoder.hip): each entry point calls the launch function stemseg_hip_encoder_forward
 * calls for that pass, so the kernel it picks is the one the pass picks.  Exported for tests and per-kernel benches.  Additive:
 * STEMSEG_HIP_ABI_VERSION stays 11.
 *   form       0 = the launch function's own choice; > 0 forces one kernel.  A forced form whose preconditions do not hold returns
 *              STEMSEG_E_INVALID with last_error and launches nothing.
 *   form_used  (may be NULL) receives the form that ran.
 * Max-pool and stride-2 copy: STEMSEG_STREAM_FORM_SCALAR (one output per thread, 64-bit grid-stride indices: any shape) or _VEC4 (four
 * outputs of a row per thread from two 16-byte loads, 32-bit indices; needs W % 8 == 0, 16-byte aligned in and out, and
 * planes * (H / 2) * (W / 8) < 2^31).  The own choice is _VEC4 wherever it applies.
 * Top-down add: STEMSEG_UP2_FORM_SCALAR (in place, any even shape), _VEC4X2 (in place; one thread = an aligned group of four columns of
 * two haloed fine rows; needs y_stride % 4 == 0, t_stride % 4 == 0, 4 * ((W + 1) / 4 + 1) <= y_stride, fine.ptr - y_stride - 1 -- the
 * haloed buffer's row 0 -- 16-byte aligned, and C * T * H * ((W + 1) / 4 + 1) < 2^32 - 256), _DENSE (the same, reading the fine term from
 * fine_dense and writing the fine buffer: also W % 4 == 0, fine_dense 16-byte aligned, and C * T * (H / 2 + 1) * ((W + 1) / 4 + 1) <
 * 2^32 - 256 in place of the last condition).  The own choice: with fine_dense, _DENSE (STEMSEG_E_INVALID where it does not apply: no
 * other form reads a dense map); without, _VEC4X2 where it applies, else _SCALAR.  All forms give the same bits. */
#define STEMSEG_STREAM_FORM_AUTO   0
#define STEMSEG_STREAM_FORM_SCALAR 1
#define STEMSEG_STREAM_FORM_VEC4   2
#define STEMSEG_UP2_FORM_SCALAR    1
#define STEMSEG_UP2_FORM_VEC4X2    2
#define STEMSEG_UP2_FORM_DENSE     3
/* out[pl][y][x] = max over the 3x3 window at stride 2, padding 1 (-inf) of in[pl]: in [planes][H][W] -> out [planes][H / 2][W / 2], H and W
 * even (resnet.py:303).  A NaN in the window gives NaN. */
int stemseg_hip_maxpool3x3s2(const float* in, int64_t planes, int32_t H, int32_t W, float* out, int32_t form, int32_t* form_used, void* stream);
/* out[pl][y][x] = in[pl][2y][2x]: in [planes][H][W] -> out [planes][H / 2][W / 2], H and W even (the shared input of a stride-2 block's conv1
 * and projection shortcut).  The encoder's own kernels; stemseg_hip_subsample2 is the training path's. */
int stemseg_hip_encoder_subsample2(const float* in, int64_t planes, int32_t H, int32_t W, float* out, int32_t form, int32_t* form_used,
                                   void* stream);
/* FPN top-down path (fpn.py:64-66): fine = (fine_dense ? fine_dense : fine) + bilinear_x2(coarse), align_corners = False.  fine
 * [C][T][H][W] and coarse [C][T][H / 2][W / 2] are the INTERIOR views of zero-haloed 2-D buffers ([C][T][H + 2][pitch], the view's ptr at
 * row 1, column 1; c_stride == T * t_stride; y_stride >= W + 2), the way the encoder passes them; H and W even.  The 16-byte forms read
 * and write whole aligned groups of the haloed rows 1 .. H: the in-place form writes a halo word back as it read it, the dense form
 * writes it as +0.  fine_dense: NULL, or a dense [C * T][H][W] map. */
int stemseg_hip_upsample2x_add(const StemsegVolume* fine, const float* fine_dense, const StemsegVolume* coarse, int32_t form, int32_t* form_used,
                               void* stream);
/* The f16x3 stem's space-to-depth pass: frames [T][3][H][W] (H, W even, 8-byte aligned) -> s2d [12][T][H / 2 + 3][W / 2 + 3] with
 * s2d[(p * 2 + q) * 3 + c][t][Y + 2][X + 2] = frames[t][c][2 Y + p][2 X + q] -- the layout of the encoder plan's slice: two halo rows and
 * columns before the data, one after, c_stride == T * t_stride.  The halo is not written (the workspace keeps it zero). */
int stemseg_hip_stem_s2d(const float* frames, int32_t T, int32_t H, int32_t W, const StemsegVolume* s2d, void* stream);
/* Debugging aid, host only: the form each streaming pass of stemseg_hip_encoder_forward takes for this descriptor, on a 16-byte aligned
 * workspace.  out[0] the max-pool, out[1..3] the stride-2 copy in front of stages 2, 3, 4 (where it runs: a stage-end tail writes that copy
 * itself), out[4..6] the top-down add of levels 4x, 8x, 16x. */
int stemseg_hip_encoder_stream_forms(const StemsegEncoderDesc* desc, int32_t out[7]);
int stemseg_hip_encoder_init_workspace(const StemsegEncoderDesc* desc, void* workspace, size_t ws_bytes, void* stream);
/* the encoder's twin of stemseg_hip_decoder_check_workspace */
int stemseg_hip_encoder_check_workspace(const StemsegEncoderDesc* desc, const void* workspace, size_t ws_bytes, int32_t* n_bad_host,
                                        int64_t* first_bad_host, void* stream);
/* frames: dense [T][3][H][W] (BGR, mean-subtracted).  out[4 * c + k], c < n_clips, k = 0..3: the four FPN maps (4x, 8x, 16x,
 * 32x) of clip c as volumes [256][clip frames][H/s][W/s] -- dense, or the interior view of the decoders' zero-haloed
 * inputs (then no copy is needed). */
int stemseg_hip_encoder_forward(const StemsegEncoderDesc* desc, const StemsegEncoderWeights* weights, const float* frames,
                                const StemsegVolume* out, void* workspace, size_t ws_bytes, void* stream);
/* The stem and the max-pool of that pass again, into the caller's buffers: stem_out dense [64][T][H/2][W/2] = relu(conv7x7 s2 + bias) and
 * pooled dense [64][T][H/4][W/4] = max_pool2d(stem_out, 3, 2, 1).  The code stemseg_hip_encoder_forward runs first, with the same
 * descriptor, weights and precision -- the space-to-depth + 4x4 convolution in f16x3 where the pass takes it, the exact fp32-MFMA stem
 * otherwise -- so the bits are the pass's.  For the stem's and layer1's backward: the pass's own slices of both maps are re-used by its
 * stage-end tails.  workspace: the pass's (only its space-to-depth slice is written).  Additive: STEMSEG_HIP_ABI_VERSION stays 11. */
int stemseg_hip_encoder_stem_forward(const StemsegEncoderDesc* desc, const StemsegEncoderWeights* weights, const float* frames, float* stem_out,
                                     float* pooled, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clustering side.
 * ---------------------------------------------------------------------------------------------- */

/* inference/main.py:93-103: per-frame running sum of seediness over the clips that contain the frame,
 * then (sum / count) > thr.  accumulate: acc = (first ? 0 : acc) + plane, n floats. */
int stemseg_hip_seediness_accumulate(float* acc, const float* plane, int64_t n, int32_t first, void* stream);
int stemseg_hip_fg_mask(const float* acc, float count, float thr, uint8_t* mask, int64_t n, void* stream);
/* The same for every frame of a sequence in one launch: acc [F][HW] holds the per-frame sums (e.g. accumulated with
 * stemseg_hip_semseg_accumulate on the 1-channel seediness maps, clip after clip), counts [F] (device) the number of clips
 * that contain each frame; mask[f][p] = acc[f][p] / counts[f] > thr, 0 where counts[f] == 0 (inference/main.py:93-103). */
int stemseg_hip_fg_mask_frames(const float* acc, const float* counts, float thr, uint8_t* mask, int32_t F, int64_t HW,
                               void* stream);

/* online_chainer.py:11-22 + :258-281 : compact the foreground voxels of a clip.
 * emb [E][V], bw [Ev][V], seed [V] dense with V = T*HW, fg uint8 [V].  Point order = flat voxel order
 * (frame-major, row-major).  Outputs: emb_out [N][E], bw_out [N][Ev], seed_out [N], voxel_index [N] (int32),
 * frame_offsets [T+1] int64 (exclusive prefix of per-frame counts; frame_offsets[T] = N).  Outputs must be
 * sized for N = V.  scratch: >= 16 * (V/1024 + 2) bytes (integer division), 8-byte aligned -- a bound on what is laid out, which with
 * nb = ceil(V / 1024) is [nb] int32 block counts, padded to a multiple of 8 bytes, then [nb + 1] int64 block offsets:
 * round_up(4 * nb, 8) + 8 * (nb + 1) bytes.  No host synchronisation. */
int stemseg_hip_fg_gather(const float* emb, const float* bw, const float* seed, const uint8_t* fg,
                          int32_t E, int32_t Ev, int32_t T, int64_t HW,
                          float* emb_out, float* bw_out, float* seed_out, int32_t* voxel_index,
                          int64_t* frame_offsets, void* scratch, void* stream);

typedef struct StemsegClusterParams {
    float   primary_prob_thresh;    /* 0.5  (clusterers.py:40)  */
    float   secondary_prob_thresh;  /* 0.3                      */
    float   min_seediness_prob;     /* 0.8 / 0.95 (KITTI)       */
    int32_t max_instances;          /* 20                       */
    int32_t n_free_dims;
    float   free_dim_bandwidths[STEMSEG_MAX_EMB_DIMS];   /* 1/std^2, computed by the caller in fp32 */
} StemsegClusterParams;

/* read-back record, written by the last kernel into caller-provided DEVICE memory (copy it to the host
 * when convenient; it is what online_chainer.py needs to continue: K and the instance list). */
typedef struct StemsegClusterMeta {
    int32_t K;                      /* instances found; instance_labels = label_start + 0..K-1 */
    int32_t exhausted;              /* loop ran max_instances rounds (stale-mask quirk active) */
    int64_t n_points;
    int64_t n_unassigned_last;      /* num_unassigned_pts at the last evaluated loop header     */
    float   centers[STEMSEG_MAX_INSTANCES][STEMSEG_MAX_EMB_DIMS];
    float   bandwidths[STEMSEG_MAX_INSTANCES][STEMSEG_MAX_EMB_DIMS];   /* cat(bw_seed, free) ; std = sqrt(clamp(1/bw)) */
    float   seed_prob[STEMSEG_MAX_INSTANCES];
} StemsegClusterMeta;

size_t stemseg_hip_cluster_workspace_bytes(int64_t n_max);
/* SequentialClustering._process (inference/clusterers.py:60-166) including its quirks.
 * emb [N][E], bw [N][Ev], seed [N]; E = Ev + n_free_dims <= 8.  n_points_dev: optional device pointer to the
 * actual N (e.g. frame_offsets + T from stemseg_hip_fg_gather) -- if NULL, N = n_max.
 * labels [n_max] int64 (-1 = unassigned).  opt_masks: NULL or uint8 [max_instances][n_max] primary match masks;
 * opt_probs: NULL or float [max_instances][n_max] per-round probabilities (0 where unavailable).
 * Enqueues max_instances + 2 kernels; no host synchronisation. */
int stemseg_hip_cluster(const float* emb, const float* bw, const float* seed, int64_t n_max,
                        const int64_t* n_points_dev, int32_t E, int32_t Ev,
                        const StemsegClusterParams* params, int64_t label_start,
                        int64_t* labels, StemsegClusterMeta* meta_dev,
                        uint8_t* opt_masks, float* opt_probs,
                        void* workspace, size_t ws_bytes, void* stream);

/* The same for several independent point sets at once -- the clips of one step: every launch of the loop serves all of them
 * (grid.y = set), so a step's clustering costs max_instances + 2 launches instead of that per clip.  Sets are independent
 * (own workspace, own record); results are bit-identical to n_items separate stemseg_hip_cluster calls.  E, Ev and params are shared. */
typedef struct StemsegClusterItem {
    const float*   emb;              /* [n_max][E] */
    const float*   bw;               /* [n_max][Ev] */
    const float*   seed;             /* [n_max] */
    int64_t        n_max;
    const int64_t* n_points_dev;     /* optional device pointer to the actual N */
    int64_t        label_start;
    int64_t*       labels;           /* [n_max] */
    StemsegClusterMeta* meta_dev;
    uint8_t*       opt_masks;
    float*         opt_probs;
    void*          workspace;        /* >= stemseg_hip_cluster_workspace_bytes(n_max) */
    size_t         ws_bytes;
} StemsegClusterItem;
int stemseg_hip_cluster_batch(const StemsegClusterItem* items, int32_t n_items, int32_t E, int32_t Ev,
                              const StemsegClusterParams* params, void* stream);

/* online_chainer.py:291-343: label-pair statistics on the overlap frames.  lut_a / lut_b map (label + 1)
 * to a row / column index or -1 (ignore; the outlier label -1 maps through slot 0).  Outputs (int64,
 * zeroed by the call): inter [Ka][Kb], cnt_a [Ka], cnt_b [Kb].  No limit on Ka, Kb or on the label values
 * (the LUTs are indexed by id): small tables are counted in LDS, large ones with global atomics. */
int stemseg_hip_overlap_counts(const int64_t* labels_a, const int64_t* labels_b, int64_t n,
                               const int32_t* lut_a, int32_t lut_a_len, const int32_t* lut_b, int32_t lut_b_len,
                               int32_t Ka, int32_t Kb, int64_t* inter, int64_t* cnt_a, int64_t* cnt_b, void* stream);

/* online_chainer.py:304-308 (`unique()` of the overlap labels) and :43-49 (`highest id + 1`) in one pass:
 * present[id] = 1 for every label id in [0, cap) that occurs, present[cap] = 1 when a NEGATIVE label (the outlier id -1) occurs
 * -- `present` holds cap + 1 bytes; the reference's id enumeration order depends on whether -1 is in the set (online_chainer.py:308-309,
 * see reference_id_order) --, *max_plus_1 = max(label) + 1 over labels >= 0 (0 when there is none; ids >= cap still count towards the maximum).  accumulate = 0 zeroes both outputs
 * first; accumulate = 1 adds to what earlier calls left (several frames' label arrays -> one id set). */
int stemseg_hip_label_presence(const int64_t* labels, int64_t n, uint8_t* present, int32_t cap,
                               int64_t* max_plus_1, int32_t accumulate, void* stream);

/* in-place relabel: labels[i] = map[labels[i] + 1] for labels[i] + 1 in [0, map_len) (online_chainer.py:219-229) */
int stemseg_hip_relabel(int64_t* labels, int64_t n, const int64_t* map, int32_t map_len, void* stream);

/* ---- clip-parallel stitching: what a rank needs when the clips of ONE sequence are clustered on different GPUs
 * (the chain itself is online_chainer.py:193-236).  A clip clustered with label_start = 1 leaves ONE BYTE per
 * voxel -- 0 background, 1..K the clip-local instance (labels are i + label_start, clusterers.py:121), 255 the outlier label
 * -1 -- and only those planes are exchanged.  "bin" below maps a code to a table index: 0..B-2 as is, 255 -> B-1,
 * B = max_instances + 2. ---- */

/* masks_to_coord_list alone (online_chainer.py:11-22): voxel_index [N] + frame_offsets [T+1] of stemseg_hip_fg_gather, without
 * the head outputs.  scratch as for stemseg_hip_fg_gather. */
int stemseg_hip_fg_compact(const uint8_t* fg, int32_t T, int64_t HW, int32_t* voxel_index, int64_t* frame_offsets, void* scratch,
                           void* stream);

/* codes[0..V) = 0, then codes[voxel_index[i]] = labels[i] - label_start + 1 (255 for labels[i] < 0), i < N; N from
 * n_points_dev (device, e.g. frame_offsets + T) or n_max when NULL. */
int stemseg_hip_labels_to_codes(const int64_t* labels, const int32_t* voxel_index, const int64_t* n_points_dev, int64_t n_max,
                                int64_t label_start, uint8_t* codes, int64_t V, void* stream);

/* online_chainer.py:291-343's statistics for every (clip, frame) of a sequence in ONE launch.  codes: [planes][HW];
 * item k compares plane_a[k] (the frame as labelled by the clip that contributed it to the track container; -1: none, every
 * voxel counts under a = 0) with plane_b[k] (the same frame as labelled by the current clip) over the voxels that are
 * foreground in plane_b: tables[k][a][b] (int32, zeroed by the call) = #voxels with bin(code_a) = a, bin(code_b) = b.
 * plane_a / plane_b: DEVICE int32 [n_items]. */
int stemseg_hip_pair_tables(const uint8_t* codes, const int32_t* plane_a, const int32_t* plane_b, int32_t n_items, int64_t HW,
                            int32_t B, int32_t* tables, void* stream);

/* The relabel of online_chainer.py:219-224 as a gather: for item k = (src_begin, count, vbase, plane, out_begin) (DEVICE int64
 * [n_items][5]): out[out_begin + q] = lut[k][bin(codes[plane][voxel_index[src_begin + q] - vbase])], q < count.
 * lut: DEVICE int64 [n_items][B] (final track id per clip-local code).  max_count = max over items of count. */
int stemseg_hip_codes_to_labels(const uint8_t* codes, const int32_t* voxel_index, const int64_t* items, int32_t n_items,
                                int64_t max_count, const int64_t* lut, int64_t HW, int32_t B, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Semantic-segmentation side (datasets with MODEL.USE_SEMSEG_HEAD: youtube_vis.yaml, kitti_mots_*.yaml).
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_MAX_CLIP_FRAMES 32
#define STEMSEG_SEMSEG_NONE 0     /* foreground probability only                                   */
#define STEMSEG_SEMSEG_LOGITS 1   /* multiclass: mean class logits, float [F][C-1][HW]            */
#define STEMSEG_SEMSEG_PROBS 2    /* multiclass: softmax over the classes, float [F][C-1][HW]     */
#define STEMSEG_SEMSEG_ARGMAX 3   /* multiclass: class index, int64 [F][HW]                       */

/* inference_model.py:121-128: acc[frame_index[t]][c][:] += clip_logits[c][t][:] for the T slots of one clip.
 * acc: [n_frames][C][HW], ZERO-initialised by the caller before the first clip (the reference starts each frame's sum from
 * the float 0., :80); clip_logits: the semseg decoder's output [C][T][HW]; frame_index: HOST array of T frame numbers, -1 =
 * skip the slot; the non-negative entries of one call must be distinct (a clip that repeats a frame, inference/main.py:37-39,
 * is accumulated with one call per repetition so that the per-frame order of the fp32 adds stays slot order, :126-128). */
int stemseg_hip_semseg_accumulate(float* acc, const float* clip_logits, int32_t C, int32_t T, int64_t HW,
                                  const int32_t* frame_index, int32_t n_frames, void* stream);

/* InferenceModel.get_semseg_masks (inference_model.py:197-231) on the accumulated sums: mean = acc / counts[f] (device
 * float [F]); C > 2: fg = sigmoid(mean[C-1]), multiclass from mean[0..C-2] per output_type; C == 2: fg = softmax(mean)[1]
 * and no multiclass output (the reference then fails on `[].cpu()`, :231 -- here the buffer is simply left untouched).
 * fg: float [F][HW]. */
int stemseg_hip_semseg_masks(const float* acc, const float* counts, int32_t F, int32_t C, int64_t HW, int32_t output_type,
                             float* fg, void* multiclass, void* stream);

/* The same for ONE clip on its own (independent clips: every frame belongs to exactly one clip, the mean over clips is the
 * clip's own logits): clip_logits [C][T][HW] -> fg_prob float [T][HW] (may be NULL) and fg_mask uint8 [T][HW] = fg_prob > thr
 * (may be NULL) -- inference_model.py:197-231 + inference/main.py:142-144 without the [F][C][HW] accumulator round trip. */
int stemseg_hip_semseg_fg_clip(const float* clip_logits, int32_t C, int32_t T, int64_t HW, float thr, float* fg_prob,
                               uint8_t* fg_mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pre-processing (inference_image_loader.py:23-43, data/common.py:12-30, structures/image_list.py:93-104), one launch:
 * frames uint8 [T][H0][W0][3] (device) -> bilinear resize to (new_h, new_w), align_corners=False -> optional / 255 ->
 * (x - mean[c]) / std[c] -> optional channel flip (RGB models) -> out float [T][3][pad_h][pad_w], zero right / bottom padding.
 * mean / std are HOST arrays of 3 floats in the frames' channel order.
 * ---------------------------------------------------------------------------------------------- */
int stemseg_hip_preprocess_frames(const uint8_t* frames, int32_t T, int32_t H0, int32_t W0, int32_t new_h, int32_t new_w,
                                  int32_t pad_h, int32_t pad_w, const float mean[3], const float std[3], int32_t unit_scale,
                                  int32_t flip_channels, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mask materialisation for the writers (output_utils/davis.py:76-110; same chain in youtube_vis.py:118-155 and
 * kitti_mots.py:89-130).  File formats stay on the host.
 * ---------------------------------------------------------------------------------------------- */

/* davis.py:76-77: dense [H][W] uint8 := 0, then dense[ys[i]][xs[i]] = lut[labels[i] + 1] -- lut maps (track label + 1) to
 * "index in instances_to_keep + 1" (1..255) or 0 for labels that are not kept (outliers, tracks beyond max_tracks). */
int stemseg_hip_scatter_instance_index(const int64_t* ys, const int64_t* xs, const int64_t* labels, int64_t n, const int32_t* lut,
                                       int32_t lut_len, uint8_t* dense, int32_t H, int32_t W, void* stream);

/* davis.py:79-110 fused: one-hot planes of `dense` [h][w] -> bilinear x mask_scale (align_corners=False) -> crop to
 * (crop_h, crop_w) = the resized network input without its zero padding -> bilinear resize to (out_h, out_w) -> > 0.5 ->
 * out [out_h][out_w] uint8 = kept-instance index + 1 (0 = none).  mask_scale = 1 reproduces `upscaled_inputs`. */
int stemseg_hip_resample_instance_masks(const uint8_t* dense, int32_t h, int32_t w, float mask_scale, int32_t crop_h, int32_t crop_w,
                                        int32_t out_h, int32_t out_w, uint8_t* out, void* stream);

/* ABI 11: the same two steps on a uint8 (index_bytes = 1, bit-identical to the calls above) or uint16 (index_bytes = 2) map, so
 * that up to 65534 kept instances fit (lut values 1..65535).  `dense` / `out` point to H*W / out_h*out_w elements of that type. */
int stemseg_hip_scatter_instance_index_ex(const int64_t* ys, const int64_t* xs, const int64_t* labels, int64_t n, const int32_t* lut,
                                          int32_t lut_len, void* dense, int32_t index_bytes, int32_t H, int32_t W, void* stream);
int stemseg_hip_resample_instance_masks_ex(const void* dense, int32_t index_bytes, int32_t h, int32_t w, float mask_scale, int32_t crop_h,
                                           int32_t crop_w, int32_t out_h, int32_t out_w, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 11: COCO RLE of condensed index maps (youtube_vis.py:118-161, kitti_mots.py:150-173; pycocotools maskApi.c semantics).
 * maps [F][H][W] of uint8 / uint16 (index_bytes), value n in 1..K = kept instance n, 0 (or > K) = none.  Plane q = f * K + n - 1
 * is the binary mask (maps[f] == n) in column-major order p = x * H + y.
 *   rle_workspace_bytes(F, H, W, K, max_changes): device workspace for at most `max_changes` plane boundaries in all (each pixel
 *     whose value differs from its column-major predecessor is a boundary of at most two planes; 2 * F * H * W always suffices).
 *   rle_plan: writes per plane the number of RLE counts (plane_counts [F*K], int32) and compressed characters (plane_chars
 *     [F*K], int64), and totals[3] = {all counts, all characters, boundaries needed} (device).  If the boundaries exceed
 *     max_changes, totals[0] = totals[1] = -1 and nothing else is valid: re-plan with max_changes >= totals[2].
 *   rle_encode (same arguments and workspace, after rle_plan on the same stream): counts [totals[0]] int32, count_offsets [F*K+1],
 *     chars [totals[1]] (rleToString, not NUL-terminated), char_offsets [F*K+1], area [F*K] (rleArea) and bbox [F*K][4]
 *     (rleToBbox: x, y, w, h).  Deterministic; a fixed number of launches (the radix passes depend on the bits of F*K only).
 * ---------------------------------------------------------------------------------------------- */
size_t stemseg_hip_rle_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t K, int64_t max_changes);
int stemseg_hip_rle_plan(const void* maps, int32_t index_bytes, int32_t F, int32_t H, int32_t W, int32_t K, int64_t max_changes,
                         void* workspace, size_t ws_bytes, int32_t* plane_counts, int64_t* plane_chars, int64_t* totals, void* stream);
int stemseg_hip_rle_encode(const void* maps, int32_t index_bytes, int32_t F, int32_t H, int32_t W, int32_t K, int64_t max_changes,
                           void* workspace, size_t ws_bytes, int32_t* counts, int64_t* count_offsets, uint8_t* chars, int64_t* char_offsets,
                           int32_t* area, int32_t* bbox, void* stream);

/* ABI 11: per-instance class statistics over the foreground points of F frames in one call (youtube_vis.py:113-126,
 * kitti_mots.py:103-119).  ys / xs / labels: all frames' points concatenated, frame f's are [frame_offsets[f], frame_offsets[f+1])
 * (device int64 [F+1]); max_frame_points bounds the largest frame (grid size).  Instance of a point: n = lut[label + 1] in 1..K.
 *   points [F][K] int64: points of instance n in frame f (mask resolution h x w).
 *   logits (nullable) float [F][C_logits][h*w]: sums [K][C_logits-1] fp64 of classes 1..C_logits-1 over all frames; partial is a
 *     [F][K][C_logits-1] fp64 scratch.  Fixed-order reductions, no float atomics: bitwise deterministic.
 *   argmax (nullable) int64 [F][h*w]: votes [K][C_votes] int64, votes[n-1][c] = points of instance n whose class is c. */
int stemseg_hip_instance_class_stats(const int64_t* ys, const int64_t* xs, const int64_t* labels, const int64_t* frame_offsets, int32_t F,
                                     int64_t max_frame_points, const int32_t* lut, int32_t lut_len, int32_t K, int32_t h, int32_t w,
                                     const float* logits, int32_t C_logits, double* partial, double* sums, const int64_t* argmax,
                                     int32_t C_votes, int64_t* points, int64_t* votes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Visualisations (save_vis: output_utils/davis.py:124-161, youtube_vis.py:193-222, kitti_mots.py:208-239).  Additive: these
 * symbols joined ABI 11 without changing any earlier entry point, so STEMSEG_HIP_ABI_VERSION stays 11.
 *   vis_composite: frames [F][H][W][3] BGR uint8, index_map [F][H][W] uint8 / uint16 (index_bytes), colors [K+1][3] uint8.  A pixel
 *     with n = index_map in 1..K gets trunc(0.6 * colors[n][c] + (1 - 0.6) * frames[c]) per channel c in fp64 (utils/vis.py
 *     overlay_mask_on_image; colors[n][0] goes to channel 0, as the reference applies its RGB palette to a BGR image); every other
 *     pixel is copied.  out may equal frames.
 *   jpeg_workspace_bytes(F, H, W): device workspace of a jpeg_plan / jpeg_encode pair for F BGR uint8 frames [F][H][W][3].
 *   jpeg_plan: baseline JFIF of every frame, byte-identical to libjpeg-turbo (PIL Image.save(..., "JPEG", quality)): 4:2:0, islow
 *     FDCT, standard tables scaled by `quality` (1..100, baseline clamp), standard Huffman tables, no restart markers.  Writes the
 *     file size of each frame (frame_bytes [F], int64) and their sum (total [1], int64), both on the device.
 *   jpeg_encode (same F, H, W, quality and workspace, after jpeg_plan on the same stream): the files back to back in out
 *     [out_bytes >= total] and offsets [F+1] int64 (file f is out[offsets[f] .. offsets[f+1])).  Deterministic; a fixed number of
 *     launches whatever F or the data.
 * ---------------------------------------------------------------------------------------------- */
int stemseg_hip_vis_composite(const uint8_t* frames, const void* index_map, int32_t index_bytes, int32_t F, int32_t H, int32_t W,
                              const uint8_t* colors, int32_t K, uint8_t* out, void* stream);
size_t stemseg_hip_jpeg_workspace_bytes(int32_t F, int32_t H, int32_t W);
int stemseg_hip_jpeg_plan(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t quality, void* workspace, size_t ws_bytes,
                          int64_t* frame_bytes, int64_t* total, void* stream);
int stemseg_hip_jpeg_encode(int32_t F, int32_t H, int32_t W, int32_t quality, void* workspace, size_t ws_bytes, uint8_t* out,
                            int64_t out_bytes, int64_t* offsets, void* stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG decode of input frames (inference_model.py:51-53 cv2.imread; generic_video_dataset_parser.py:61-72).  Additive: these
 * symbols joined ABI 11 without changing any earlier entry point, so STEMSEG_HIP_ABI_VERSION stays 11.
 * Output pixel-identical to libjpeg-turbo's default decompression (islow IDCT, fancy upsampling, table-driven YCbCr -> RGB; PIL
 * Image.open(...).convert("RGB") and cv2.imread(..., IMREAD_COLOR)) for single-scan SOF0 / SOF1 Huffman files with 8-bit samples:
 * one component (replicated to B = G = R) or YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; any size, any restart interval.
 * F frames of one geometry per call; each frame has its own tables.
 *   sampling: 0 = one component, else (luma h << 4) | luma v: 0x11, 0x21 or 0x22.
 *   data: the frames' files (or just their entropy-coded segments) back to back; ecs_offsets [F][2] int64: frame f's entropy-coded
 *     segment is data[ecs_offsets[2f] .. ecs_offsets[2f+1]) (after the SOS header, before the final EOI).
 *   tables [F][7872] uint8, one blob per frame (stemseg_amd/utils/jpeg.py builds it, little-endian):
 *     [0, 64)     int32 hdr[16]: restart interval in MCUs (0 = none), components, DC table of component c at hdr[2+c], AC table at
 *                 hdr[5+c], quant table at hdr[8+c]
 *     [64, 576)   uint16 quant[4][64], natural (row-major) order
 *     [576, ...)  8 Huffman tables (DC 0..3, AC 0..3) of 912 bytes: uint16 look[256] ((length << 8) | symbol of the code in the
 *                 next 8 bits, 0 = longer code), int32 maxcode[18] (largest code of each length, -1 if none), int32 valoff[18]
 *                 (index of the first code of each length in vals, minus that code), uint8 vals[256]
 *   total_bytes >= the sum of the segment lengths, total_intervals >= the sum over frames of ceil(MCUs / restart interval): they
 *     size the workspace and the grids (a frame past them is flagged corrupt).
 *   sub_bits (0 = 512): the Huffman subsequence length in bits, a multiple of 64; max_rounds (0 = 256): the bound on the
 *     synchronisation rounds inside a workgroup.  Small values force the multi-round and the serial-backstop paths (tests).
 *   jpeg_decode_workspace_bytes(F, H, W, sampling, total_bytes, total_intervals, sub_bits): device workspace; 0 on bad arguments.
 *   jpeg_decode: out [F][H][W][3] BGR uint8; status [F] uint8: bit 0 = corrupt (an invalid code, k > 63, a segment exhausted inside a
 *     block, a wrong RST sequence, a stray marker, an interval with the wrong number of blocks) -- that frame's pixels are undefined
 *     and libjpeg's "repair" is not attempted: decode it on the host; bit 1 = the synchronisation took more than one round; bit 2 =
 *     the serial backstop decoded it.  A fixed number of launches whatever the data; no host synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t stemseg_hip_jpeg_decode_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t sampling, int64_t total_bytes, int64_t total_intervals,
                                               int32_t sub_bits);
int stemseg_hip_jpeg_decode(const uint8_t* data, const int64_t* ecs_offsets, const uint8_t* tables, int32_t F, int32_t H, int32_t W,
                            int32_t sampling, int64_t total_bytes, int64_t total_intervals, int32_t sub_bits, int32_t max_rounds,
                            void* workspace, size_t ws_bytes, uint8_t* out, uint8_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG decode of input frames (the KITTI-MOTS frames; inference_model.py:51-53 cv2.imread).  Additive: these symbols joined ABI 11
 * without changing any earlier entry point, so STEMSEG_HIP_ABI_VERSION stays 11.
 * Output pixel-identical to libpng (cv2.imread(..., IMREAD_COLOR)) and PIL Image.open(...).convert("RGB") for non-interlaced files
 * with bit depth 8 and colour type 0 (gray, replicated to B = G = R), 2 (RGB), 4 (gray + alpha) or 6 (RGBA); alpha is dropped.
 * F frames of one geometry per call.
 *   channels: 1, 2, 3 or 4 (colour types 0, 4, 2, 6).
 *   data: the frames' zlib streams (each its IDAT payloads concatenated) back to back, followed by 8 readable bytes; offsets
 *     [F + 1] int64: frame f's stream is data[offsets[f] .. offsets[f + 1]).
 *   headers (stemseg_amd/utils/png.py builds it, little-endian): int64 hdr[F][8] = {H, W, channels, stream length, first IDAT
 *     record, IDAT count, 0, 0}, then uint32 idat[N][4] = {payload offset in the frame's stream, payload length, stored chunk CRC,
 *     frame}, in frame order.  N <= total_bytes + F.  A header that disagrees with the call or the offsets marks the frame corrupt.
 *   total_bytes >= offsets[F]: sizes the workspace and the grids.
 *   sub_bits (0 = 512): the subsequence length in bits of the wave decode of a Huffman block, a multiple of 64 in [64, 65536];
 *     small values force several synchronisation rounds (tests).
 *   flags: bit 0 turns the block finder off, so the serial backstop decodes every block (tests and A/B runs); other bits must be 0.
 *   png_decode_workspace_bytes(F, H, W, channels, total_bytes, sub_bits, flags): device workspace, about 5 * F * H * (1 + W *
 *     channels) + 6 * total_bytes bytes; 0 on bad arguments (F, H or W < 1, H or W > 65535, channels not 1..4, total_bytes < 0 or
 *     >= 2^32, a bad sub_bits, an unknown flag, H * (1 + W * channels) >= 2^31).
 *   png_decode: out [F][H][W][3] BGR uint8; status [F] uint8: bit 0 = corrupt (a wrong IDAT CRC or Adler-32, a bad zlib header,
 *     an invalid block header or code, BTYPE 11, a stored length mismatch, a distance before the start of the stream or beyond the
 *     window, a missing final block, bytes after the Adler-32, an inflated length other than H * (1 + W * channels), a row filter
 *     type > 4) -- that frame's pixels are undefined: decode it on the host; bit 1 = the synchronisation of a block's wave decode took
 *     more than one round; bit 2 = the serial backstop decoded at least one block.
 *     A fixed number of launches whatever the data; no host synchronisation.  Returns STEMSEG_E_INVALID on the argument errors
 *     above, a null pointer or a workspace smaller than png_decode_workspace_bytes.
 * ---------------------------------------------------------------------------------------------- */
size_t stemseg_hip_png_decode_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t channels, int64_t total_bytes, int32_t sub_bits,
                                              int32_t flags);
int stemseg_hip_png_decode(const uint8_t* data, const int64_t* offsets, const void* headers, int32_t F, int32_t H, int32_t W,
                           int32_t channels, int64_t total_bytes, int32_t sub_bits, int32_t flags, void* workspace, size_t ws_bytes,
                           uint8_t* out, uint8_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding loss and its gradient with respect to the head output (modeling/losses/embedding_loss.py:10-185 on the Lovasz hinge,
 * modeling/losses/_lovasz.py:51-63,130-147).  Additive: these symbols joined ABI 11 without changing any earlier entry point, so
 * STEMSEG_HIP_ABI_VERSION stays 11.  One sample per call; its instances are a grid dimension, so the number of launches (14 forward,
 * 3 backward) does not depend on the instance count or the volume.  No floating-point atomics: two runs give identical bits.
 *   embedding_map [C][T][H][W] fp32, C = E + (E - n_free_dims) + 1: tanh + grid embeddings, RAW bandwidth channels, sigmoid seediness.
 *   masks [I][T][H][W] uint8 / bool (0 or 1; instances may overlap), ignore_masks [T][H][W] uint8 / bool.
 *   free_dim_bandwidths[k] = 1 / std_k^2 of free dim k (embedding dim E - n_free_dims + k), computed by the caller in fp32.
 *   The reference's pairing is reproduced: the n-th PRESENT (non-empty) instance's centre and mean bandwidth are paired with masks[n],
 *   the n-th instance overall, for n below the number of present instances K; a pair whose masks[n] is empty is skipped.
 *   Sort order of the Lovasz errors: descending error, ties by ascending voxel index.
 *   embedding_loss_workspace_bytes: device workspace of a forward / backward pair (about 24 * I * T * H * W bytes); 0 on bad arguments.
 *   Practical volume: the sort works in tiles of 4096 voxels and every workgroup of a scatter pass sums the digit histograms of all
 *     nt = ceil(T * H * W / 4096) tiles of its instance (256 * nt reads; nt^2 * 256 per instance and pass).  That is negligible at the
 *     training shape (nt = 51) and stays small against the pass itself up to about 2^21 voxels (nt = 512); the calls accept up to
 *     2^24 - 1 voxels and stay correct there, but a pass then reads billions of histogram words per instance: split such a volume.
 *   embedding_loss_forward: out (device, double [4]) = { sum over kept pairs of the Lovasz hinge, the sample's smoothness term (already
 *     divided by K), background + foreground seediness terms, K }; all zeros when the sample has no mask point.  The caller combines
 *     samples: lovasz / total K, smoothness / N, seediness / (total K + 1).  counts_host (nullable, int32 [2]): when given, the call
 *     SYNCHRONISES the stream and writes { K, kept pairs } -- the one readback, the reference's divisors depend on it.
 *   embedding_loss_backward (same descriptor, inputs and workspace, after the forward on the same stream): grad [C][T][H][W] :=
 *     d (upstream[0] * lovasz / total_instances + upstream[1] * smoothness / batch_size + upstream[2] * seediness / (total_instances + 1))
 *     / d embedding_map, every element written once; upstream is a device float [3].  No host synchronisation.
 *   Returns STEMSEG_E_INVALID on a descriptor of the wrong size, embedding_size outside 1..STEMSEG_MAX_EMB_DIMS, n_free_dims outside
 *   0..embedding_size - 1, n_instances outside 1..1024, T * H * W outside 1..2^24 - 1, a null pointer or a workspace that is too small.
 * ---------------------------------------------------------------------------------------------- */
typedef struct StemsegEmbeddingLossDesc {
    int32_t struct_bytes;        /* = sizeof(StemsegEmbeddingLossDesc), checked */
    int32_t embedding_size;      /* E */
    int32_t n_free_dims;
    int32_t n_instances;         /* I: rows of masks */
    int32_t T, H, W;
    int32_t reserved;            /* 0 */
    float   free_dim_bandwidths[STEMSEG_MAX_EMB_DIMS];
} StemsegEmbeddingLossDesc;
size_t stemseg_hip_embedding_loss_workspace_bytes(const StemsegEmbeddingLossDesc* desc);
int stemseg_hip_embedding_loss_forward(const StemsegEmbeddingLossDesc* desc, const float* embedding_map, const uint8_t* masks,
                                       const uint8_t* ignore_masks, void* workspace, size_t ws_bytes, double* out, int32_t* counts_host,
                                       void* stream);
int stemseg_hip_embedding_loss_backward(const StemsegEmbeddingLossDesc* desc, const float* embedding_map, const uint8_t* masks,
                                        const uint8_t* ignore_masks, void* workspace, size_t ws_bytes, const float* upstream,
                                        int32_t total_instances, int32_t batch_size, float* grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training targets, the semseg cross-entropy and the foreground loss with their gradient with respect to the semseg head's output
 * (modeling/model_builder.py:128-152,210-244, modeling/losses/cross_entropy.py:9-48, data/common.py:195-210).  Additive to ABI 11.
 * One sample per call; no floating-point atomics, two runs give identical bits; no call synchronises the stream.
 *   prepare_targets (1 launch): masks [I][T][H][W] and ignore_masks [T][H][W] (uint8 / bool, 0 or 1) at full resolution ->
 *     masks_out [I][T][h][w], ignore_out [T][h][w] (uint8 0 / 1) and semseg_out [T][h][w] (uint8 class ids), h = H / 4, w = W / 4
 *     rounded down.  An output pixel is the AND of source pixels (4y + 1, 4x + 1), (4y + 2, 4x + 1), (4y + 1, 4x + 2), (4y + 2, 4x + 2):
 *     what bilinear interpolation by 1/4 (align_corners = False) followed by a cast to uint8 gives on a 0 / 1 mask.  semseg_out is the
 *     largest category_ids[i] (device int32 [I]) over the instances whose downscaled mask is set, 0 where none is.  flag (device
 *     int32) := 1 if a category id is negative or above 255, else 0.  n_instances may be 0 (masks, category_ids, masks_out unused).
 *   semseg_loss_*: logits fp32, n_classes K class channels (2..STEMSEG_MAX_SEMSEG_CLASSES, or 0: the foreground channel alone) then, if
 *     has_foreground_channel, one foreground channel; element (c, t, y, x)
 *     is at logits[c * stride_c + t * stride_t + y * stride_h + x * stride_w] (the decoder's [C][T][h][w], or any view of it), and the
 *     gradient is written with the same strides.  semseg_mask [T][H][W] uint8 class ids, ignore_mask [T][H][W] uint8 / bool, dense.
 *   semseg_loss_forward (2 launches): out (device, double [4]) = { sum over voxels of log-sum-exp - logit[target], T * H * W,
 *     sum over non-ignored voxels of the binary cross-entropy of the foreground channel against [target > 0] (0 without that channel),
 *     non-ignored voxels }.  The cross-entropy is NOT masked by ignore_mask (the reference reduces it with 'mean' before it multiplies):
 *     the caller's loss is out[0] / out[1], NaN when out[3] == 0 as in the reference; the foreground loss is out[2] / out[3].
 *     flag (device int32) := 1 if a target id is >= n_classes (such a voxel adds no cross-entropy term and is never indexed with).
 *   semseg_loss_backward (1 launch; same descriptor, inputs and workspace, after the forward on the same stream): every element of grad
 *     written once: class channels (softmax - [c == target]) * upstream[0] / batch_size / out[1], foreground channel
 *     (sigmoid - [target > 0]) * nonignore * upstream[1] / batch_size / out[3]; all NaN when out[3] == 0, as autograd gives for the
 *     reference.  upstream is a device float [2].  The workspace keeps the per-voxel log-sum-exp (4 bytes / voxel).
 *   Returns STEMSEG_E_INVALID on a descriptor of the wrong size, n_classes out of range, bad dims or strides,
 *   a null pointer, a misaligned pointer or a workspace that is too small.
 * ---------------------------------------------------------------------------------------------- */
typedef struct StemsegTargetPrepDesc {
    int32_t struct_bytes;        /* = sizeof(StemsegTargetPrepDesc), checked */
    int32_t n_instances;         /* I: rows of masks, 0..1024 */
    int32_t T, H, W;             /* full resolution, H and W at least 4 */
    int32_t reserved;            /* 0 */
} StemsegTargetPrepDesc;
typedef struct StemsegSemsegLossDesc {
    int32_t struct_bytes;        /* = sizeof(StemsegSemsegLossDesc), checked */
    int32_t n_classes;           /* K */
    int32_t has_foreground_channel;   /* 0 | 1: channel K of the logits */
    int32_t T, H, W;
    int32_t reserved;            /* 0 */
    int32_t reserved2;           /* 0 (keeps the strides 8-byte aligned) */
    int64_t stride_c, stride_t, stride_h, stride_w;   /* elements */
} StemsegSemsegLossDesc;
int stemseg_hip_prepare_targets(const StemsegTargetPrepDesc* desc, const uint8_t* masks, const uint8_t* ignore_masks,
                                const int32_t* category_ids, uint8_t* masks_out, uint8_t* ignore_out, uint8_t* semseg_out, int32_t* flag,
                                void* stream);
size_t stemseg_hip_semseg_loss_workspace_bytes(const StemsegSemsegLossDesc* desc);
int stemseg_hip_semseg_loss_forward(const StemsegSemsegLossDesc* desc, const float* logits, const uint8_t* semseg_mask,
                                    const uint8_t* ignore_mask, void* workspace, size_t ws_bytes, double* out, int32_t* flag, void* stream);
int stemseg_hip_semseg_loss_backward(const StemsegSemsegLossDesc* desc, const float* logits, const uint8_t* semseg_mask,
                                     const uint8_t* ignore_mask, void* workspace, size_t ws_bytes, const float* upstream, int32_t batch_size,
                                     float* grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the decoders' tails: everything behind the last 3x3x3 convolution of a branch -- GroupNorm -> ReLU -> (average pool), the
 * trilinear up-sampling and the 1x1x1 heads, in the folded form  heads(x) = act(up(up(up(M32 y32) + M16 y16) + M8 y8) + M4 y4 + b)  of
 * StemsegDecoderWeights.head_w (csrc/decoder_backward.hip).  Additive to ABI 11.  No floating-point atomics: a sum across workgroups
 * goes through fp64 partials in the workspace and one fixed-order combine, every slot written by every call (the workspace needs no
 * initialisation), so two runs give identical bits.  No call synchronises the stream or allocates (graph-capture safe).  Workspaces
 * are 256-byte aligned; the *_workspace_bytes queries return 0 on bad arguments (stemseg_hip_last_error says which).
 * ---------------------------------------------------------------------------------------------- */

/* One level of the folded linear tail, forward:  out[o, v] = sum_c w[o][c] x[c, v] (+ add[o, v]),  x dense [Cin][V], out and add dense
 * [n_out][V], any V, n_out <= STEMSEG_MAX_HEAD_OUT; no bias, no activation (what stemseg_hip_decoder_forward runs per coarse level). */
int stemseg_hip_level_head(const float* x, int32_t Cin, int64_t V, const float* w, int32_t n_out, const float* add, float* out,
                           void* stream);

/* Backward of stemseg_hip_heads (and of stemseg_hip_level_head), V = T * H * W of any value:
 *     dz[o, v] = d_out[o, v] * act_o'     from the forward output `out`: codes 0 / 4: 1; 1: 0.25 (1 - tanh^2), tanh = out - grid;
 *                                         2: out (1 - out); 3: out
 *     dx[c, v] = sum_o w[o][c] dz[o, v]   (dx NULL: skipped)
 *     dw[o][c] = sum_v dz[o, v] x[c, v],  db[o] = sum_v dz[o, v]   (db NULL: skipped)
 * act_host == grid_axis_host == NULL: d_out IS dz and `out` is not read -- a level matrix of the folded tail, whose activation sits
 * behind the sum of the four levels.  `bias` is not read (`out` carries it); the argument mirrors the forward call.  n_out <=
 * STEMSEG_MAX_HEAD_OUT, Cin % 4 == 0, Cin <= 512.  16-byte loads and stores along v when V % 4 == 0 and the maps are 16-byte aligned.
 * 3 launches (2 without an activation table). */
size_t stemseg_hip_heads_backward_workspace_bytes(int32_t Cin, int32_t n_out, int64_t V);
int stemseg_hip_heads_backward(const float* x, int32_t Cin, int32_t T, int32_t H, int32_t W, const float* w, const float* bias,
                               int32_t n_out, const int32_t* act_host, const int32_t* grid_axis_host, const float* grid_t,
                               const float* grid_y, const float* grid_x, const float* out, const float* d_out, float* dx,
                               float* dw, float* db, void* workspace, size_t ws_bytes, void* stream);

/* The same level matrix and its backward for a WIDE linear head, STEMSEG_MAX_HEAD_OUT < n_out <= STEMSEG_MAX_WIDE_HEAD_OUT (the 42-channel
 * YouTube-VIS semseg head), on v_mfma_f32_32x32x2_f32: exact products, fp32 accumulation, the library's "f32" arithmetic.  No activation
 * table (a wide head is raw class logits).  w is the plain dense row-major [n_out][Cin] matrix, not packed and not padded: the rows
 * n_out .. of the last 32-row MFMA block are zeros made inside the kernels, never read from memory, and nothing depends on a packed-weight
 * cache.  Additive to ABI 11.  x dense [Cin][V], dz / out / add dense [n_out][V], any V (no alignment rule), Cin % 4 == 0, Cin <= 512,
 * 0 < V < 2^40; each violation is an argument error naming the entry point and the value, before any launch.
 *     forward:   out[o, v] = sum_c w[o][c] x[c, v] (+ add[o, v], add may be NULL)                                       1 launch
 *     backward:  dx[c, v] = sum_o w[o][c] dz[o, v]   (dx NULL: skipped)
 *                dw[o][c] = sum_v dz[o, v] x[c, v],  db[o] = sum_v dz[o, v]   (db NULL: skipped)                         2 launches
 * The backward reads x once: a tile of x and dz is staged in LDS and feeds both products.  dw: fp32 sums over 16 voxels, fp64 from
 * there on; the voxel chunks' fp64 partials (stemseg_hip_wide_heads_backward_chunks of them, a function of the shape only) lie in the
 * workspace, every slot written by every call, and one thread per (o, c) adds them in chunk order.  No floating-point atomics; two runs
 * give the same bits.  The workspace is 256-byte aligned and stemseg_hip_wide_heads_backward_workspace_bytes large (STEMSEG_E_WORKSPACE
 * otherwise); the two queries return 0 on bad arguments. */
int stemseg_hip_wide_level_head(const float* x, int32_t Cin, int64_t V, const float* w, int32_t n_out, const float* add, float* out,
                                void* stream);
size_t stemseg_hip_wide_heads_backward_workspace_bytes(int32_t Cin, int32_t n_out, int64_t V);
int stemseg_hip_wide_heads_backward_chunks(int32_t Cin, int32_t n_out, int64_t V);
int stemseg_hip_wide_heads_backward(const float* x, int32_t Cin, int64_t V, const float* w, int32_t n_out, const float* dz, float* dx,
                                    float* dw, float* db, void* workspace, size_t ws_bytes, void* stream);

/* The exact adjoint of stemseg_hip_upsample_trilinear (align_corners = False, border clamping): d_out dense [C][T st][H sy][W sx] ->
 * d_in dense [C][T][H][W].  Gather form: every input voxel sums the outputs that read it, with the forward's weights, in fixed order
 * (t, y, x), in fp64, rounded once.  st 1 or 2 and sy == sx 2 or 4 (the decoders' up-samplings); anything else is an argument error.
 * 1 launch, no workspace. */
int stemseg_hip_upsample_trilinear_backward(const float* d_out, int32_t C, int32_t T, int32_t H, int32_t W, int32_t st, int32_t sy,
                                            int32_t sx, float* d_in, void* stream);

/* Backward of stemseg_hip_gn_relu_pool for pool 0 (none) and 1 (average); 2 (max) is an argument error.  x the conv output, dense
 * [C][T][H][W]; stats, gamma, beta as in the forward; d_out dense [C][To][H][W], To = pool ? (T + 1) / 2 : T.
 *     dy = pool^T(d_out) [y > 0]      y the forward's own relu(fma(x, rstd gamma, beta - mean rstd gamma)); the gradient at 0 is 0
 *     dgamma[c] = sum_v dy xhat,  dbeta[c] = sum_v dy,  xhat = (x - mean) rstd
 *     dx = rstd (gamma dy - mean_g(gamma dy) - xhat mean_g(gamma dy xhat))      means over the group's channels and voxels
 * groups == 0 (NORMALIZATION_LAYER 'none': mean 0, rstd 1, gamma 1, beta 0): dx = dy, no parameter gradients; stats, gamma, beta,
 * dgamma, dbeta and the workspace may be NULL.  16-byte accesses when W % 4 == 0 and the maps are 16-byte aligned.  3 launches. */
size_t stemseg_hip_gn_relu_pool_backward_workspace_bytes(int32_t C, int32_t T, int32_t H, int32_t W, int32_t groups);
int stemseg_hip_gn_relu_pool_backward(const float* x, int32_t C, int32_t T, int32_t H, int32_t W, int32_t groups, const float* stats,
                                      const float* gamma, const float* beta, int32_t pool, const float* d_out, float* dx,
                                      float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the tap convolutions, padding 1, stride 1 (csrc/conv_backward.hip): the weight and bias gradients, and the tap gather of the
 * data gradient, of the decoders' 3x3x3 convolution over a volume (conv3d_*, 27 taps) and of the encoder's 2-D convolutions over F
 * independent frames (conv2d_*: Conv2d(3, padding 1), taps 9, and a 1x1 convolution, taps 1).  One family: the 9-tap weight gradient is
 * the 27-tap kernel without its temporal taps.  Additive to ABI 11, under the rules of the tail's backward above:
 * v_mfma_f32_32x32x2_f32 on the fp32 operands (exact products, fp32 accumulation within a chunk of K = T H W, never a split mode: gradients
 * have no bounded magnitude), fp64 partials in the workspace, every slot written by every call, one fixed-order combine, no
 * floating-point atomics, no synchronisation, no allocation; two runs give identical bits.
 *     27 taps: dw[co][ci][kt][ky][kx] = sum_{t, y, x} dy[co][t, y, x] * x[ci][t + kt, y + ky, x + kx]      (x in haloed coordinates)
 *     taps 9:  dw[co][ci][ky][kx]     = sum_{f, y, x} dy[co][f, y, x] * x[ci][f, y + ky, x + kx]           (x in haloed coordinates)
 *     taps 1:  dw[co][ci]             = sum_{f, y, x} dy[co][f, y, x] * x[ci][f, y, x]
 *     db[co] = sum_{t, y, x} dy[co][t, y, x]                                                               (db NULL: skipped)
 * 27 taps: x_haloed is the zero-haloed view of the convolution's input (extents T + 2, H + 2, W + 2).  taps 9: x is the view that is
 * zero-haloed in y and x only, extents [Cin][F][H + 2][W + 2] (there is no halo between frames and no tap crosses them).  The halo is read
 * as it lies; zeros make the convolution a padding = 1 one.  taps 1: x is any view [Cin][F][H][W], dense or strided.  Cin = x->C, F = x->T.
 * Every view is held to one rule: its strides hold its extents (a channel's last frame and a frame's last row may stop at their last
 * element) and every element lies below its limit.  dy dense [Cout][T][H][W]; dw dense [Cout][Cin][3][3][3], [Cout][Cin][3][3] or
 * [Cout][Cin] (nn.Conv3d.weight, nn.Conv2d.weight).  The forward's channel rules: Cin % 4 == 0, Cout % 32 == 0; taps other than 1 and 9 are
 * an argument error of the conv2d calls.  The workspace and chunk functions take the OUTPUT map's H and W.  *_wgrad_chunks: the number of
 * K chunks, a function of (Cin, Cout, taps, T, H, W) only (negative: an error code).  2 launches.
 * The data gradient needs no convolution kernel of its own:  dx[ci][u] = sum_k sum_co w[co][ci][k] dy[co][u - k + 1]  is one 1x1x1
 * stemseg_hip_conv3d of the flat dy with the taps Cin x Cout matrix W_all[(k, ci)][co] = w[co][ci][k] (Cout terms per result) and a gather:
 * stemseg_hip_conv3d_col2vol sums the (at most) 27 in-range taps of every input voxel from cols = dense [27][Cin][T][H][W],
 * stemseg_hip_conv2d_col2img the (at most) 9 of every pixel of its own frame from cols = dense [9][Cin][F][H][W], in tap order, in fp64;
 * col2img then adds addend[ci][f, y, x] (dense [Cin][F][H][W]; NULL: nothing) to that sum; one rounding into dx dense [Cin][T][H][W].
 * 1 launch, no workspace.  The 3x3x3 forward kernel on flipped, transposed weights computes the same function with all 27 Cout products
 * in one fp32 accumulator, at 2 - 10 times the rounding error. */
size_t stemseg_hip_conv3d_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t T, int32_t H, int32_t W);
int stemseg_hip_conv3d_wgrad_chunks(int32_t Cin, int32_t Cout, int32_t T, int32_t H, int32_t W);
int stemseg_hip_conv3d_wgrad(const StemsegVolume* x_haloed, const float* dy, int32_t Cout, float* dw, float* db, void* workspace,
                             size_t ws_bytes, void* stream);
int stemseg_hip_conv3d_col2vol(const float* cols, int32_t Cin, int32_t T, int32_t H, int32_t W, float* dx, void* stream);
size_t stemseg_hip_conv2d_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t taps, int32_t F, int32_t H, int32_t W);
int stemseg_hip_conv2d_wgrad_chunks(int32_t Cin, int32_t Cout, int32_t taps, int32_t F, int32_t H, int32_t W);
int stemseg_hip_conv2d_wgrad(const StemsegVolume* x, const float* dy, int32_t Cout, int32_t taps, float* dw, float* db, void* workspace,
                             size_t ws_bytes, void* stream);
int stemseg_hip_conv2d_col2img(const float* cols, int32_t Cin, int32_t F, int32_t H, int32_t W, const float* addend, float* dx,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * The weight gradient of the grouped / strided 3x3 convolution (csrc/conv_backward.hip): conv2 of a ResNeXt bottleneck (stride 1 or 2) and
 * the one-group stride-2 conv2 of STRIDE_IN_1X1 = False -- the backward of stemseg_hip_conv2d_grouped.  Additive to ABI 11, under the
 * rules of the family above: v_mfma_f32_16x16x4_f32 on the fp32 operands (exact products, never a split mode), F Ho Wo cut into chunks
 * whose length is a function of the shape only, no fp32 chain longer than 16 pixels, fp64 partials in the workspace -- every slot written
 * by every call -- and one fixed-order combine that rounds once; no floating-point atomics, no allocation, no synchronisation; two runs
 * give identical bits.  2 launches.
 *     dw[co][cj][ky][kx] = sum_{f, y, x} dy[co][f, y, x] * x[g(co) Cg + cj][f, s y + ky, s x + kx]          (x in haloed coordinates)
 * with Cg = C / groups and g(co) = co / Cg.  x_haloed: the y/x-zero-haloed view [C][F][H + 2][W + 2] of the convolution's input, the
 * view stemseg_hip_conv2d_grouped reads (held to the rule of the views above); C must equal x_haloed->C.  dy dense [C][F][Ho][Wo],
 * Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1 (odd H and W allowed); dw dense [C][Cg][3][3] (nn.Conv2d(groups=).weight).  The shapes
 * of the forward: C % 16 == 0; Cg in 4, 8, 16, 32, 64 for more than one group, any multiple of 16 for one; stride 1 or 2.  With 4 or 8
 * channels per group a 16 x 16 block of the kernel holds 4 or 2 groups: the products of different groups are discarded, never stored, so a
 * NaN or inf in one group's input reaches no other group's dw.  There is no bias gradient (the FrozenBN shift is a buffer).
 * *_workspace_bytes (0: unsupported shape, see stemseg_hip_last_error) and *_chunks (the number of K chunks; negative: an error code) are
 * pure host functions of (C, groups, stride, F, H, W) with H and W the INPUT map's extents.  The workspace is 256-byte aligned.
 * The data gradient needs no kernel of its own: it is stemseg_hip_conv2d_grouped, stride 1, of dy (zero-dilated to H x W for stride 2) with
 * the per-group transposed, tap-flipped weight W'[g Cg + cj][co_j][ky][kx] = w[g Cg + co_j][cj][2 - ky][2 - kx] (stemseg_amd/hip.py
 * conv2d_grouped_dgrad). */
size_t stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(int32_t C, int32_t groups, int32_t stride, int32_t F, int32_t H, int32_t W);
int stemseg_hip_conv2d_grouped_wgrad_chunks(int32_t C, int32_t groups, int32_t stride, int32_t F, int32_t H, int32_t W);
int stemseg_hip_conv2d_grouped_wgrad(const StemsegVolume* x_haloed, const float* dy, int32_t C, int32_t groups, int32_t stride, float* dw,
                                     void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The streaming kernels of the bottleneck backward (csrc/bottleneck_backward.hip; conv2d_col2img_relu with its gather in csrc/conv_backward.hip).  Additive to ABI 11.  Maps are [C][F][H][W] over F
 * independent frames, "dense" means contiguous in that order.  Each call is 1 launch: 4 elements of a row per thread where the row
 * length is a multiple of 4 and the pointers keep 16-byte alignment, 1 otherwise.  No floating-point atomics, no allocation, no
 * synchronisation; every argument is checked before the launch, and the message names it.
 *   relu_backward:  out = (y <= 0) ? 0 : (g + addend) -- torch's threshold_backward of the fp32 sum: a NaN in y lets the gradient
 *       through, +-0.0 blocks it.  y: any view whose strides hold its extents (dense, or the interior of the y/x-zero-haloed layout);
 *       g, addend (NULL: none) and out dense [y->C][y->T][y->H][y->W]; out may be g.
 *   conv2d_col2img_relu:  stemseg_hip_conv2d_col2img with that mask applied to the fp64 sum (taps, then the addend) before its one
 *       rounding: bit for bit relu_backward(mask, col2img(cols, addend)).  mask: a view [Cin][F][H][W], e.g. the interior of the haloed
 *       conv2 input.
 *   subsample2:  in dense [C][F][H][W] -> out dense [C][F][H/2][W/2], the even rows and columns.  H and W (of the LARGE map, in both
 *       calls) must be even.
 *   scatter2:  its adjoint with an addend: g dense [C][F][H/2][W/2] -> out dense [C][F][H][W] = addend + g at (even y, even x); elsewhere
 *       the addend's own bits, or zeros without one (addend NULL).
 *   scale_rows:  dw[r][0 .. row_len) *= scale[r], in place.
 *   sum_partials:  out[i] = parts[0][i] + ... + parts[n - 1][i] (+ addend[i]), summed in fp64 in that order and rounded once; parts dense
 *       [n][N], addend (NULL: none) and out dense [N].  The K chunks of a 1x1 data gradient over many channels. */
int stemseg_hip_relu_backward(const StemsegVolume* y, const float* g, const float* addend, float* out, void* stream);
int stemseg_hip_conv2d_col2img_relu(const float* cols, int32_t Cin, int32_t F, int32_t H, int32_t W, const float* addend,
                                    const StemsegVolume* mask, float* dx, void* stream);
int stemseg_hip_subsample2(const float* in, int32_t C, int32_t F, int32_t H, int32_t W, float* out, void* stream);
int stemseg_hip_scatter2(const float* g, int32_t C, int32_t F, int32_t H, int32_t W, const float* addend, float* out, void* stream);
int stemseg_hip_scale_rows(float* dw, const float* scale, int32_t rows, int64_t row_len, void* stream);
int stemseg_hip_sum_partials(const float* parts, int32_t n, int64_t N, const float* addend, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The backward of the stem (csrc/stem_backward.hip): the max-pool's adjoint and the 7x7 stride-2 convolution's weight gradient.  Additive
 * to ABI 11.  No floating-point atomics, no allocation, no synchronisation; two runs give identical bits.
 *   maxpool3x3s2_backward:  dx [planes][H][W] = the adjoint of max_pool2d(x, 3, 2, 1) applied to g [planes][H/2][W/2]; x [planes][H][W]
 *       the pool's input, H and W even.  Gather form, 1 launch: every input pixel looks at the (at most 2 x 2) windows that contain it,
 *       recomputes each window's arg-max by torch's rule -- rows, then columns, of the window clipped to the map; a value replaces the
 *       running one when it is greater or a NaN, so the first maximum and the last NaN win -- and adds g where the arg-max is the pixel
 *       itself, in ascending (oy, ox) order, in fp32 from +0: torch's CPU backward bit for bit.  mask_relu = 1: a pixel with x <= 0 then
 *       gets 0 by relu_backward's rule (a NaN in x lets the gradient through, +-0.0 blocks it): the adjoint of the ReLU in front of the
 *       pool, in the same pass.  form / form_used as for stemseg_hip_maxpool3x3s2: STEMSEG_STREAM_FORM_SCALAR (one pixel per thread) or
 *       _VEC4 (the 2 x 4 pixels of two rows per thread, from 35 input values held in registers, two 16-byte stores: W % 4 == 0 and 16-byte
 *       aligned x and dx; the own choice where it applies).  Both forms give the same bits.
 *   stem_wgrad:  dw [64][3][7][7] = the weight gradient of Conv2d(3, 64, 7, stride 2, padding 3) over F frames,
 *           dw[co][c][ky][kx] = sum_{f, oy, ox} g[co][f][oy][ox] * frames[f][c][2 oy + ky - 3][2 ox + kx - 3]       (0 outside the frame)
 *       frames dense [F][3][H][W], H and W even; g dense [64][F][H/2][W/2].  Under the rules of the weight gradients above:
 *       v_mfma_f32_32x32x2_f32 on the fp32 operands (exact products, never a split mode), F Ho Wo cut into chunks whose length is a
 *       function of (F, H, W) only (at most 8 tiles of 4 x 32 output pixels: no fp32 chain is longer than 256 products), fp64 partials
 *       [chunk][64][147] in the workspace -- every slot written by every call -- and one fixed-order combine (sixteen runs of consecutive
 *       chunks, each in chunk order, then the runs in order) that rounds once.  2 launches.  There is no bias gradient (the FrozenBN shift is a buffer) and no data
 *       gradient (the input is the frames).  *_workspace_bytes (0: unsupported shape, see stemseg_hip_last_error) and *_chunks (the number
 *       of K chunks; negative: an error code) are pure host functions of (F, H, W).  The workspace is 256-byte aligned. */
int stemseg_hip_maxpool3x3s2_backward(const float* x, const float* g, int64_t planes, int32_t H, int32_t W, int32_t mask_relu, float* dx,
                                      int32_t form, int32_t* form_used, void* stream);
size_t stemseg_hip_stem_wgrad_workspace_bytes(int32_t F, int32_t H, int32_t W);
int stemseg_hip_stem_wgrad_chunks(int32_t F, int32_t H, int32_t W);
int stemseg_hip_stem_wgrad(const float* frames, const float* g, int32_t F, int32_t H, int32_t W, float* dw, void* workspace, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * The optimiser step, the global gradient norm and the clip coefficient (training/utils.py:195-210: torch.optim.SGD / Adam over
 * model.parameters(); torch.nn.utils.clip_grad_norm_).  csrc/optimizer.hip: one launch over every tensor of a parameter group.
 *
 * Tables, both in DEVICE memory, 8-byte aligned, built once per parameter group and kept while pointers, sizes and flags stay:
 *   tensors [n_tensors] of StemsegOptTensor: p (the parameter, updated in place), g (its gradient, read only), state1 / state2 (SGD: the
 *     momentum buffer / unused; Adam: exp_avg / exp_avg_sq; NULL where the optimiser keeps none), n elements (fp32, dense), flags:
 *     STEMSEG_OPT_STATE_UNINIT = state1 holds nothing yet -- the SGD step then WRITES buf = g without reading it (torch's first step).
 *   chunks [n_chunks] of StemsegOptChunk { tensor, chunk }: chunk k of tensor t is its elements [k * STEMSEG_OPT_CHUNK,
 *     min(n, (k + 1) * STEMSEG_OPT_CHUNK)).  THE CHUNK RULE: tensors in table order, each tensor's chunks in rising order, ceil(n /
 *     STEMSEG_OPT_CHUNK) of them (none for n = 0) -- a chunk never straddles tensors and every element lies in exactly one, so the
 *     table is a function of the sizes alone.  stemseg_hip_opt_plan (host only, no HIP call) checks a HOST copy of the descriptors and
 *     writes the chunk table to host memory (chunks_host NULL: counts only); the caller uploads both.  n_states: 0, 1 or 2 state
 *     pointers must be non-NULL.  A kernel skips a table entry that does not lie inside its tensor.
 * Launch: min(n_chunks, 2048) workgroups stride over the chunk table; 16-byte loads and stores where p, g and the states in use are all
 * 16-byte aligned, scalars otherwise and for the last n % 4 elements; same bits either way; nothing at or past element n is written.
 * Hyper-parameters by value (StemsegOptHyper), so a new learning rate needs no new table.  Per element, each operation rounded to fp32
 * where torch's CPU kernels round (fma: one rounding):
 *   sgd_step (torch/optim/sgd.py _single_tensor_sgd):  g *= *grad_scale (pointer given);  g = fma(wd, p, g) (wd != 0);  momentum != 0:
 *     buf = g on STATE_UNINIT, else buf = fma(1 - dampening, g, buf * momentum);  g = nesterov ? fma(momentum, buf, g) : buf;
 *     p = fma(-lr, g, p).  With momentum == 0 no state pointer is touched.
 *   adam_step (torch/optim/adam.py _single_tensor_adam, L2 weight decay, no amsgrad):  g *= *grad_scale;  g = fma(wd, p, g);
 *     m = fma(1 - beta1, g - m, m);  v = fma((1 - beta2) * g, g, v * beta2);  p = p + (-step_size * m) / (sqrt(v) / bc2_sqrt + eps), with
 *     tensor_scalars (device, float [n_tensors][2]) = { step_size = lr / bias_correction1, bc2_sqrt = sqrt(bias_correction2) } of each
 *     tensor's own step count, computed by the host as torch does.
 *   g is never written.  grad_scale: NULL or a device float read by the kernel (the coef below): no host synchronisation.
 *   grad_norm (2 launches): partials [n_chunks] double and partial_flags [n_chunks] int32 := per chunk the fp64 sum of g * g (every square
 *     exact) and 1 if an element is inf or NaN; then *norm (double) = sqrt of their sum, added in a fixed order -- each of 256 threads a run of
 *     consecutive chunks, the runs in a tree --, *flag (int32) = OR of the flags, *coef (float) = min(1, max_norm / (norm + 1e-6))
 *     (clip_grad_norm_'s clip_coef_clamped); max_norm < 0: coef = 1.  Only g and n of the descriptors are read.
 * No floating-point atomics: two runs give the same bits.  STEMSEG_E_INVALID before any HIP call on: a NULL table or output, n_tensors
 * <= 0, n_chunks <= 0, a negative n, an unknown flag (descriptor or hyper-parameters), a struct of the wrong size, a missing state
 * pointer, a misaligned pointer, a NaN max_norm.
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_OPT_CHUNK 16384          /* elements per chunk: 64 KiB of each array, 16 float4 rounds of a 256-thread workgroup */
#define STEMSEG_OPT_STATE_UNINIT 1       /* StemsegOptTensor.flags: the momentum buffer is not yet initialised */
#define STEMSEG_OPT_NESTEROV 1           /* StemsegOptHyper.flags */
typedef struct {
    float*       p;
    const float* g;
    float*       state1;
    float*       state2;
    int64_t      n;
    int32_t      flags;
    int32_t      reserved;               /* 0 */
} StemsegOptTensor;
typedef struct {
    int32_t tensor, chunk;
} StemsegOptChunk;
typedef struct {
    int32_t struct_bytes;                /* sizeof(StemsegOptHyper) */
    int32_t flags;
    float   lr, momentum, one_minus_dampening, weight_decay;      /* SGD (weight_decay: Adam too) */
    float   one_minus_beta1, beta2, one_minus_beta2, eps;         /* Adam; the differences taken in double by the host, as torch does */
} StemsegOptHyper;
int stemseg_hip_opt_plan(const StemsegOptTensor* tensors_host, int32_t n_tensors, int32_t n_states, StemsegOptChunk* chunks_host,
                         int64_t chunks_cap, int64_t* n_chunks);
int stemseg_hip_opt_sgd_step(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                             const StemsegOptHyper* hyper, const float* grad_scale, void* stream);
int stemseg_hip_opt_adam_step(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                              const StemsegOptHyper* hyper, const float* tensor_scalars, const float* grad_scale, void* stream);
int stemseg_hip_opt_grad_norm(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                              double* partials, int32_t* partial_flags, double max_norm, double* norm, float* coef, int32_t* flag,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * The gradient bucket of data-parallel training (the reference wraps its model in DistributedDataParallel, training/main.py): one flat,
 * averaged gradient that every rank holds bit for bit, which the step and the norm above then read in place.  csrc/optimizer.hip; the
 * tables are StemsegOptTensor / StemsegOptChunk under THE CHUNK RULE, the launch is min(n_chunks, 2048) workgroups striding over the
 * chunk table, 16-byte accesses where both sides are 16-byte aligned, scalars otherwise and for the last n % 4 elements, the same bits
 * either way.  Additive: STEMSEG_HIP_ABI_VERSION stays 11.
 *
 *   THE LAYOUT RULE (opt_bucket_plan; host only, no HIP call): offset[t] = the sum of round_up(n, 4) over the tensors before t, total =
 *     that sum over all tensors.  Every slice of a 16-byte-aligned bucket is therefore 16-byte aligned, and the layout is a function of
 *     the sizes alone: the same on every rank.  offsets_host NULL: the total only.  Only n of the descriptors is read.
 *   pack_grads: bucket[offset[t] + i] = g_t[i] * scale, one fp32 multiply; with scale == 1.0f the bits are copied (NaN payloads, -0.0 and
 *     denormals included).  A descriptor whose g is NULL writes +0.0f over its slice -- the only entry point that accepts a NULL g -- and
 *     the up-to-3 padding elements behind every slice are written +0.0f, so the whole of [0, total) is defined after one call.  g is
 *     never written, unless it IS the slice (a gradient accumulated in place), which is then scaled in place.  p and the states are not
 *     read.  offsets: device, int64 [n_tensors], 8-byte aligned; bucket: device, fp32 [total], 16-byte aligned.
 *   unpack_grads: the reverse copy, p_t[i] = bucket[offset[t] + i], where the caller's table has p := the destination (as grad_norm's has
 *     p := g): a parameter broadcast, or gradients for an optimiser that wants them apart.  A NULL p is skipped.  g is not read.
 *   reduce_ranks: gathered fp32 [world][total] (an all-gather of every rank's bucket) -> bucket[i] = (float)((double(gathered[0][i]) +
 *     double(gathered[1][i]) + ...) / (double)world): fp64 additions in rising rank order, one division, one rounding to fp32; inf and NaN
 *     propagate.  world 1 .. STEMSEG_OPT_MAX_WORLD.  Any total > 0; the bucket must not lie inside gathered.
 * Nothing outside [0, total) of the bucket, or outside [0, n) of a p, is written; a kernel skips a slice that its offset does not keep
 * inside the bucket.  No floating-point atomics.  STEMSEG_E_INVALID before any HIP call on: a NULL table, offsets, bucket or output,
 * n_tensors <= 0, n_chunks <= 0, a negative n (bucket_plan), a bucket not 16-byte aligned (reduce_ranks: 4-byte), offsets or a table
 * not 8-byte aligned, a total that is not the plan's -- not a positive multiple of 4, or outside the range that n_chunks chunks over
 * n_tensors tensors can hold, (n_chunks - n_tensors) * CHUNK < total <= n_chunks * CHUNK (the descriptors are in device memory: the
 * host sees their sizes through the counts alone) --, world outside its range, a scale that is inf or NaN.
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_OPT_MAX_WORLD 64
int stemseg_hip_opt_bucket_plan(const StemsegOptTensor* tensors_host, int32_t n_tensors, int64_t* offsets_host, int64_t* total);
int stemseg_hip_opt_pack_grads(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                               const int64_t* offsets, float* bucket, int64_t total, float scale, void* stream);
int stemseg_hip_opt_unpack_grads(const StemsegOptTensor* tensors, int32_t n_tensors, const StemsegOptChunk* chunks, int64_t n_chunks,
                                 const int64_t* offsets, const float* bucket, int64_t total, void* stream);
int stemseg_hip_opt_reduce_ranks(const float* gathered, int32_t world, int64_t total, float* bucket, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The device half of the training data loader (the reference's data/video_dataset.py): annotation strings -> binary planes -> the
 * network's mask size.  csrc/data_loader.hip.  Additive: STEMSEG_HIP_ABI_VERSION stays 11.
 * The same parse also serves the evaluations: rle_decode_labels (KITTI-MOTS) and rle_pair_inter (YouTube-VIS: string against string, no plane).
 *
 *   rle_decode: M COCO RLE strings, concatenated in `chars` (device) with offsets_host[M + 1] (host, int64, from 0 to n_chars), are
 *     decoded with pycocotools' rleFrString + rleDecode into planes uint8 [P][H][W] (device, 0 / 1, row-major): string m fills plane
 *     plane_of_string_host[m] (host, int32, distinct, < P).  Every byte of `planes` is written by every call: a plane that no string
 *     names is zero, and so is the plane of a string that is refused.  status uint8 [M] (device) is 0, or the FIRST of these checks
 *     that the string fails, in this order:
 *       STEMSEG_RLE_EMPTY      the string has no character
 *       STEMSEG_RLE_BAD_CHAR   a character outside 48 .. 111
 *       STEMSEG_RLE_OPEN_GROUP the last character has the "more follows" bit 0x20 set
 *       STEMSEG_RLE_BAD_COUNT  a count that is negative after its delta, or that no plane can hold: above H * W, a delta beyond
 *                              +-2^31, or one written in more than 12 characters
 *       STEMSEG_RLE_BAD_SUM    the counts do not sum to H * W
 *     Integers only, no atomics; the only stores into `planes` are at the storing thread's own pixel index, so no string can move a
 *     write.  The two host arrays are read by the argument checks alone, before the call returns; the kernels read `offsets` (int64
 *     [M + 1], 8-byte aligned) and `plane_of_string` (int32 [M]), the caller's device copies of the same values, which it uploads as
 *     it sees fit (one pinned staging buffer with the characters, say) -- the call itself copies nothing.
 *     16 launches, whatever M, P and the data; no copy, no synchronisation.
 *   rle_decode_union: rle_decode's arguments, with one change to the contract: plane_of_string may name a plane MORE than once, and
 *     must not decrease, so that the strings of one plane are contiguous (M may exceed P).  planes[p] is the OR of the decodes of the
 *     accepted strings that name p; a plane nobody names is zero; a refused string contributes nothing to its plane and gets the status
 *     byte rle_decode gives it (same checks, same order).  Every byte of `planes` is written, each by the thread of that pixel, once:
 *     no plane per string exists anywhere, so the memory does not grow with the strings of a plane (the Mapillary ignore mask is the
 *     union of up to hundreds of segments of a 5 - 20 MP image).  Workspace: rle_decode_union_workspace_bytes(n_chars, M, P).
 *     15 launches, whatever M, P and the data; integers only, no atomics, no copy, no synchronisation.
 *   resize_masks: planes uint8 [P][H0][W0] -> out uint8 [P + n_ranges][pad_h][pad_w]: out[q, :new_h, :new_w] = bilinear(planes[q],
 *     (new_h, new_w), align_corners=False) > 0.5 by torch's rule (scale = float(in) / out, source index clamped at 0, W then H, unfused
 *     fp32), zero elsewhere (the reference's BinaryMask.resize and pad_masks_to_image).  Output plane P + r is the same resize of
 *     1 - any(planes[start_r + k * stride_r], k < count_r), taken at full resolution, union_ranges_host holding (start, count, stride)
 *     per range (host, int32 [n_ranges][3], read before the call returns).  flip_x: the source columns mirrored.  One launch.
 * STEMSEG_E_INVALID with last_error, before any HIP call, on: a null pointer, M < 0, P < M, H * W >= 2^31, n_chars outside [0, 2^30),
 * offsets that do not run from 0 to n_chars without decreasing, misaligned device tables, a plane index >= P, two strings naming one plane
 * (rle_decode; rle_decode_union instead: plane indices that decrease, and no P < M), a workspace below
 * rle_decode_workspace_bytes(n_chars, M, P) (which returns 0 for arguments it refuses); a union range that leaves [0, P), more than
 * STEMSEG_MAX_UNION_RANGES ranges, pad < new.
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_RLE_EMPTY       1
#define STEMSEG_RLE_BAD_CHAR    2
#define STEMSEG_RLE_OPEN_GROUP  4
#define STEMSEG_RLE_BAD_COUNT   8
#define STEMSEG_RLE_BAD_SUM    16
#define STEMSEG_MAX_UNION_RANGES 64
size_t stemseg_hip_rle_decode_workspace_bytes(int64_t n_chars, int32_t M, int32_t P);
int stemseg_hip_rle_decode(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* plane_of_string_host,
                           const int64_t* offsets, const int32_t* plane_of_string, int32_t M, int32_t P, int32_t H, int32_t W, void* workspace,
                           size_t ws_bytes, uint8_t* planes, uint8_t* status, void* stream);
size_t stemseg_hip_rle_decode_union_workspace_bytes(int64_t n_chars, int32_t M, int32_t P);
int stemseg_hip_rle_decode_union(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* plane_of_string_host,
                                 const int64_t* offsets, const int32_t* plane_of_string, int32_t M, int32_t P, int32_t H, int32_t W,
                                 void* workspace, size_t ws_bytes, uint8_t* planes, uint8_t* status, void* stream);
int stemseg_hip_resize_masks(const uint8_t* planes, int32_t P, int32_t H0, int32_t W0, int32_t new_h, int32_t new_w, int32_t pad_h, int32_t pad_w,
                             const int32_t* union_ranges_host, int32_t n_ranges, int32_t flip_x, uint8_t* out, void* stream);
/*   rle_decode_labels: rle_decode_union's arguments and contract for the strings (plane_of_string must not decrease; same parse, same
 *     status checks in the same order), plus a label per string: label_of_string_host (host, int32 [M], 1 .. 65535, read by the
 *     argument checks alone) and label_of_string (device, int32 [M], 4-byte aligned, the same values).  The planes are LABEL MAPS:
 *       maps    uint16 [P][H][W] (device, row-major): maps[p] at a pixel is the LARGEST label among the accepted strings of plane p whose
 *               decode is 1 there, else 0.  A refused string contributes nothing and gets its status byte.
 *       overlap int32 [P] (device): the number of pixels of plane p that more than one accepted string covers.
 *     Every element of `maps` and `overlap` is written by every call; each pixel is stored by its own thread, once; no plane per string
 *     exists anywhere.  `overlap` is filled with zeros by a launch of its own, then summed through a workgroup reduction and one integer
 *     atomic per workgroup and plane: the same bits in every run.  Workspace: rle_decode_labels_workspace_bytes(n_chars, M, P) (0 for
 *     arguments it refuses).  16 launches, whatever M, P and the data; integers only, no copy, no synchronisation.
 *     STEMSEG_E_INVALID with last_error, before any HIP call, on what rle_decode_union refuses, a label outside 1 .. 65535, and `maps`
 *     not 2-byte or `overlap` or `label_of_string` not 4-byte aligned. */
size_t stemseg_hip_rle_decode_labels_workspace_bytes(int64_t n_chars, int32_t M, int32_t P);
int stemseg_hip_rle_decode_labels(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* plane_of_string_host,
                                  const int32_t* label_of_string_host, const int64_t* offsets, const int32_t* plane_of_string,
                                  const int32_t* label_of_string, int32_t M, int32_t P, int32_t H, int32_t W, void* workspace, size_t ws_bytes,
                                  uint16_t* maps, int32_t* overlap, uint8_t* status, void* stream);
/*   rle_pair_inter: rle_decode's strings (chars, offsets_host, offsets: M strings of one H x W; same parse, same status checks in the
 *     same order) and a list of PAIRS of them: pairs (device, int32 [n_pairs][2], 4-byte aligned) and pairs_host (host, the same values,
 *     read by the argument checks alone), each two string indices in [0, M); a pair may repeat and may name one string twice.
 *       status uint8 [M]       (device): the status byte of each string, as rle_decode gives it.
 *       area   int32 [M]       (device): the number of 1-pixels of string m; 0 for a refused string.
 *       inter  int32 [n_pairs] (device): the number of pixels that are 1 in BOTH strings of pair k; 0 when either is refused.
 *     Every element of all three is written by every call.  NO plane and no buffer proportional to H * W exists anywhere: the
 *     intersection is taken on the runs (the thread at the end of a 1-run of the pair's longer string searches the other string for the
 *     run that covers its start and walks forward until a run starts past its end), so the work grows with the strings' runs, and the
 *     workspace, rle_pair_inter_workspace_bytes(n_chars, M, n_pairs) (0 for arguments it refuses), with n_chars and M alone.  Integers
 *     only; no atomics: a workgroup per pair (per string for `area`), summed through shuffles and LDS, each inter[k] and area[m] stored
 *     once by one thread, so the results are fixed by the data.  A refused string is never walked, and a walk never leaves the
 *     character range of its string, so malformed strings cannot move a write or lengthen a walk.  15 launches, whatever M, the pairs
 *     and the data; no copy, no synchronisation.  M = 0 with n_pairs = 0 is valid.  This is the device half of the YouTube-VIS
 *     measures below.
 *     STEMSEG_E_INVALID with last_error, before any HIP call, on: a null pointer, M < 0, n_pairs < 0, H or W < 1, H * W >= 2^31,
 *     n_chars outside [0, 2^30), offsets that do not run from 0 to n_chars without decreasing, device offsets not 8-byte aligned,
 *     `pairs`, `area` or `inter` not 4-byte aligned, a pair index outside [0, M), a workspace that is too small. */
size_t stemseg_hip_rle_pair_inter_workspace_bytes(int64_t n_chars, int32_t M, int32_t n_pairs);   /* 0 for arguments it refuses */
int stemseg_hip_rle_pair_inter(const uint8_t* chars, int64_t n_chars, const int64_t* offsets_host, const int32_t* pairs_host,
                               const int64_t* offsets, const int32_t* pairs, int32_t M, int32_t n_pairs, int32_t H, int32_t W,
                               void* workspace, size_t ws_bytes, int32_t* area, int32_t* inter, uint8_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Geometric augmentation of a uint8 frame and its instance planes on the device (the reference's data/image_to_seq_augmenter.py and
 * data/instance_duplicator.py, which use imgaug and cv2.warpAffine).  csrc/augment.hip.  Additive: STEMSEG_HIP_ABI_VERSION stays 11.
 * The transforms are DEFINED here (DESIGN.md section 9p lists the departures from cv2 / imgaug); tests/augment_oracle.py restates them.
 * Integers, unfused fp32 and fp64 only, no atomics; every kernel stores at the storing thread's own output index alone, checks a source
 * index before it reads, and writes every byte of every output (no memset needed).  One launch each; no copy, no synchronisation.
 *
 *   warp_clip: src uint8 [H][W][3] and planes uint8 [N][H][W] (0 <= N <= STEMSEG_WARP_MAX_PLANES; planes may be NULL when N == 0) ->
 *     F warped frames.  hinv: double [F][9] (device, 8-byte aligned), frame f's INVERSE homography, output pixel (x, y) -> source
 *     (u, v) = ((h0 x + h1 y) + h2, (h3 x + h4 y) + h5) / d, d = (h6 x + h7 y) + h8, in unfused fp64; d <= 1e-12 (or not a number):
 *     the pixel is outside.  jitter: int32 [F][3] (device) = (add, hs, flags), STEMSEG_JITTER_ADD / STEMSEG_JITTER_HUE_SAT.
 *       frames  uint8 [F][H][W][3]: bilinear over the taps (floor(u) + {0,1}, floor(v) + {0,1}) with a zero border, each tap the
 *               JITTERED source pixel, fp32 weights from the fp64 fractions, floor(value + 0.5).
 *       invalid uint8 [F][H][W]: 1 where the weights of the taps inside the frame sum to < 0.5.
 *       out_planes uint8 [N][F][H][W]: out_planes[n] = (n == winner), winner the highest n with planes[n] != 0 at the nearest
 *               source pixel (floor(u + 0.5), floor(v + 0.5)); all zero where that pixel is outside.
 *     jitter of a pixel (b, g, r), a pure uint8 -> uint8 function: with STEMSEG_JITTER_ADD, c = clamp(c + add, 0, 255) per channel;
 *     then with STEMSEG_JITTER_HUE_SAT, to 8-bit HSV (H in [0,180), S and V in [0,255], rounded to nearest), H = (H + trunc(hs * 180 /
 *     255)) mod 180, S = clamp(S + hs, 0, 255), and back, rounded to nearest -- unfused fp32 in the operation order of csrc/warp.h.
 *   motion_blur: frames uint8 [F][H][W][3] -> out (another buffer of the same shape): frame f correlated with the ksize[f] x ksize[f]
 *     matrix in taps[f][0 .. k * k) (fp32 [F][STEMSEG_BLUR_MAX_K^2], row-major, device), border reflect-101, the fp32 sum of
 *     tap * pixel in row-major tap order (unfused), floor(sum + 0.5) clamped to 0..255.  ksize 0: the frame is copied.  ksize_host: int32
 *     [F] on the HOST, checked and passed to the kernel by value (so F <= STEMSEG_BLUR_MAX_FRAMES), read before the call returns.
 *   duplicate_instance: frames uint8 [T][H][W][3], mask uint8 [T][H][W] -> frames_out (same shape), masks_out uint8 [2][T][H][W]
 *     (plane 0: the original instance without what the copy covers, plane 1: the copy).  params: int32 [T][8] (device) = (has_box, xmin,
 *     ymin, xmax, ymax (exclusive maxima), flip, shift_x, shift_y (the BITS of two floats)).  Pixel (x, y) reads the source
 *     (x - shift_x, y - shift_y) (fp64, exact) bilinearly with a zero border; with flip, a tap inside the box reads column
 *     xmin + xmax - 1 - x' instead.  m = floor(bilinear(mask != 0) + 0.5); masks_out[1] = m, masks_out[0] = m ? 0 : mask,
 *     frames_out = m ? floor(bilinear(frames) + 0.5) : frames.  A frame with has_box == 0 is copied, its mask into both planes.
 *   preprocess_frames_masked: stemseg_hip_preprocess_frames with invalid uint8 [T][H0][W0]: the value is the bilinear resize of
 *     normalise(pixel) * (1 - invalid) -- a pixel whose four taps are all valid is computed exactly as preprocess_frames computes it.
 * STEMSEG_E_INVALID with last_error, before any HIP call, on: a null pointer, a dimension < 1, F or T < 1, N outside
 * 0 .. STEMSEG_WARP_MAX_PLANES, a frame of 2^31 pixels or more, a misaligned hinv, F above STEMSEG_BLUR_MAX_FRAMES, a ksize that is even, negative or above
 * STEMSEG_BLUR_MAX_K, H or W <= ksize / 2, out == frames.
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_WARP_MAX_PLANES 127
#define STEMSEG_JITTER_ADD       1
#define STEMSEG_JITTER_HUE_SAT   2
#define STEMSEG_BLUR_MAX_K      11
#define STEMSEG_BLUR_MAX_FRAMES 128
int stemseg_hip_warp_clip(const uint8_t* src, const uint8_t* planes, int32_t N, int32_t H, int32_t W, const double* hinv, const int32_t* jitter,
                          int32_t F, uint8_t* frames, uint8_t* out_planes, uint8_t* invalid, void* stream);
int stemseg_hip_motion_blur(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const int32_t* ksize_host, const float* taps, uint8_t* out,
                            void* stream);
int stemseg_hip_duplicate_instance(const uint8_t* frames, const uint8_t* mask, int32_t T, int32_t H, int32_t W, const int32_t* params,
                                   uint8_t* frames_out, uint8_t* masks_out, void* stream);
int stemseg_hip_preprocess_frames_masked(const uint8_t* frames, const uint8_t* invalid, int32_t T, int32_t H0, int32_t W0, int32_t new_h,
                                         int32_t new_w, int32_t pad_h, int32_t pad_w, const float mean[3], const float std[3],
                                         int32_t unit_scale, int32_t flip_channels, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The integer half of the DAVIS region (J) and boundary (F) measures, for all frames of one sequence in one launch
 * (csrc/davis_eval.hip; stemseg_amd/evaluation/davis.py divides the tables on the host in fp64).  Additive: STEMSEG_HIP_ABI_VERSION
 * stays 11.  The arithmetic is DEFINED here -- it follows the published DAVIS 2017 protocol, and its agreement with the official
 * toolkit's numbers is unverified -- and restated in numpy by tests/davis_eval_oracle.py.
 *
 *   pred: index map [T][H][W] (device), uint8 (index_bytes = 1) or uint16 (2).  Labels 1 .. Kp are the proposals; 0 and everything
 *     above Kp is background.  gt: uint8 planes [Kg][T][H][W] (device), non-zero = member of object g (the layout rle_decode yields);
 *     planes may overlap.
 *   A pixel (y, x) is a BOUNDARY pixel of a binary mask m iff m[y][x] differs from m at (y, x + 1), (y + 1, x) or (y + 1, x + 1), the
 *     neighbour coordinates clamped to the frame (so the bottom-right pixel never is one); boundary pixels may lie outside the mask.
 *   near(m) is the boundary map dilated by the disk dx^2 + dy^2 <= r^2; outside the frame there is nothing.
 *   counts: int32, seven tables in this order, T frames each (stemseg_hip_davis_eval_counts_size(T, Kp, Kg) elements in all; it returns
 *     0 for arguments it refuses):
 *       inter  [T][Kp][Kg]  pixels of proposal p inside object g
 *       m_p    [T][Kp][Kg]  boundary pixels of p inside near(g)
 *       m_g    [T][Kp][Kg]  boundary pixels of g inside near(p)
 *       area_p [T][Kp]      pixels of p            n_p [T][Kp]  boundary pixels of p
 *       area_g [T][Kg]      pixels of g            n_g [T][Kg]  boundary pixels of g
 *     Every element is written by every call (a fill launch, then the counting launch: 2 launches whatever the data).
 * Integers only -- sums of ones through integer atomics, which do not depend on their order: two runs give the same bits.  No float, no
 * copy, no synchronisation.  A frame's counts depend on that frame alone.
 * STEMSEG_E_INVALID with last_error, before any HIP call, on: a null pointer, index_bytes not 1 or 2, T outside
 * 1 .. STEMSEG_DAVIS_EVAL_MAX_FRAMES, H or W < 1, H * W >= 2^31, H > 16 * 65535, Kp outside 1 .. STEMSEG_DAVIS_EVAL_MAX_PROPOSALS, Kg outside
 * 1 .. STEMSEG_DAVIS_EVAL_MAX_OBJECTS, r outside 1 .. STEMSEG_DAVIS_EVAL_MAX_RADIUS, a misaligned pointer, counts_size below the size above.
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_DAVIS_EVAL_MAX_PROPOSALS 64
#define STEMSEG_DAVIS_EVAL_MAX_OBJECTS   32
#define STEMSEG_DAVIS_EVAL_MAX_RADIUS    32
#define STEMSEG_DAVIS_EVAL_MAX_FRAMES    65535
int64_t stemseg_hip_davis_eval_counts_size(int32_t T, int32_t Kp, int32_t Kg);
int stemseg_hip_davis_eval_counts(const void* pred, int32_t index_bytes, const uint8_t* gt, int32_t T, int32_t H, int32_t W, int32_t Kp, int32_t Kg,
                                  int32_t r, int32_t* counts, int64_t counts_size, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The device half of the KITTI-MOTS measures sMOTSA, MOTSA and MOTSP (csrc/mots_eval.hip and rle_decode_labels above;
 * stemseg_amd/evaluation/mots.py keeps the integer bookkeeping and the fp64 divisions).  Additive: STEMSEG_HIP_ABI_VERSION stays 11.
 * The measure is DEFINED here, after Voigtlaender et al., "MOTS: Multi-Object Tracking and Segmentation", CVPR 2019; its agreement with
 * the numbers of the official mots_tools is UNVERIFIED.  tests/mots_eval_oracle.py restates it on dense numpy masks.
 *
 *   Classes 1 (car) and 2 (pedestrian) are evaluated separately, totals over all sequences.  Per frame t and class c: H_t the result
 *   masks of class c with non-zero area, G_t the ground-truth masks of class c with non-zero area, I_t the union of the ground-truth
 *   masks of the ignore class (10 in MOTS txt files; category 3 of a video-dataset json).  The masks of one side of one frame, ignore
 *   included, must be pairwise disjoint (the evaluator refuses a frame where `overlap` is not 0).  Result masks of other classes are left
 *   out.  h and g MATCH iff 3 * inter > area_h + area_g (IoU > 0.5, in integers); disjoint masks match at most once each.
 *     TP = matched pairs; FN = |G_t| - TP_t; an unmatched h is IGNORED iff 2 * |h n I_t| > area_h, else it is an FP;
 *     IDS = matched g whose ground-truth track was last matched, in any earlier frame, to another result track id; M = sum_t |G_t|;
 *     TPs = math.fsum of the matched pairs' inter / (area_h + area_g - inter) in fp64.
 *     sMOTSA = (TPs - FP - IDS) / M, MOTSA = (TP - FP - IDS) / M, MOTSP = TPs / TP; a zero denominator gives 0.0.
 *
 *   label_pair_counts: a, b uint16 label maps [T][H][W] (device; what rle_decode_labels yields) -> counts int32 [T][Ka + 1][Kb + 1]:
 *     counts[t][i][j] = the number of pixels of frame t with a == i and b == j.  Row and column 0 are the background; a label above Ka
 *     (Kb) counts as 0.  So every frame's table sums to H * W, the areas are the marginals and the intersections with ignore labels
 *     are ordinary cells.  Ka, Kb in 1 .. STEMSEG_LABEL_PAIR_MAX_LABELS (the table of a workgroup lies in LDS: 64 x 64 int32).
 *     Every element is written by every call: a fill launch, then the counting launch (2 launches whatever the data).  Sums of ones
 *     through LDS integer atomics -- one add of the lane count per wave, step and distinct pair, never 64 adds on one word -- and one
 *     global integer atomic per non-zero cell and workgroup: two runs give the same bits.  No float, no copy, no synchronisation.
 *     A frame's table depends on that frame alone.
 * STEMSEG_E_INVALID with last_error, before any HIP call, on: a null pointer, T < 1, H or W < 1, H * W >= 2^31, Ka or Kb outside
 * 1 .. STEMSEG_LABEL_PAIR_MAX_LABELS, a misaligned pointer, counts_size below stemseg_hip_label_pair_counts_size(T, Ka, Kb) (which
 * returns 0 for arguments it refuses), T * ceil(H * W / 8192) >= 2^31.
 * ---------------------------------------------------------------------------------------------- */
#define STEMSEG_LABEL_PAIR_MAX_LABELS 63
int64_t stemseg_hip_label_pair_counts_size(int32_t T, int32_t Ka, int32_t Kb);   /* T*(Ka+1)*(Kb+1), 0 if refused */
int stemseg_hip_label_pair_counts(const uint16_t* a, const uint16_t* b, int32_t T, int32_t H, int32_t W,
                                  int32_t Ka, int32_t Kb, int32_t* counts, int64_t counts_size, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The YouTube-VIS measures AP, AP50, AP75, AR1 and AR10 (mask AP over TRACKS).  The device half is rle_pair_inter above
 * (csrc/data_loader.hip); stemseg_amd/evaluation/ytvis.py sums the integers over the frames, matches and accumulates on the host in
 * fp64.  No new entry point.  The measure is DEFINED here: it is COCOeval's (Lin et al., "Microsoft COCO: Common Objects in Context",
 * ECCV 2014, and the pycocotools evaluate / accumulate / summarize steps) lifted to tracks as Yang et al., "Video Instance
 * Segmentation", ICCV 2019 describe; the youtubevos cocoapi and the evaluation server are not available to this project, so its
 * agreement with their numbers is UNVERIFIED.  tests/ytvis_eval_oracle.py restates it on dense numpy masks.
 *
 *   A result track has a video, a score, a category and T masks (some missing: empty); a ground-truth track a category, iscrowd
 *   (default 0) and T masks.  Track IoU of result d and ground truth g: I = sum_t inter_t, U = sum_t (area_d,t + area_g,t - inter_t),
 *   for a crowd g U = sum_t area_d,t; iou = I / U in fp64, 0.0 when U = 0.  Pairs only within one video and one category.
 *   IoU thresholds linspace(0.5, 0.95, 10), recall thresholds linspace(0, 1, 101), maxDets (1, 10, 100).  NO area ranges.
 *   Matching per (video, category): results by score descending (stable), the first 100; ground truth non-crowd first (stable); per
 *   threshold t every result in turn takes the ground truth of highest IoU >= the running bound (which starts at min(t, 1 - 1e-10))
 *   among those not taken (a crowd may be taken again), never trading a non-crowd match for a crowd one; a result matched to a crowd
 *   is ignored; an unmatched one is an FP.
 *   Accumulation per (category, threshold, maxDet): from every video the first maxDet results of that one matching, merged by score
 *   (descending, stable); cumulative TP and FP over the non-ignored; recall = TP / n_gt (the non-crowd ground-truth tracks), precision
 *   = TP / (TP + FP + spacing(1)), made monotone from the right and sampled at the 101 recall points with searchsorted(side="left"),
 *   0 beyond the last.  A category with n_gt = 0 is left out.
 *   AP = the mean over thresholds, categories and recall points at maxDet 100; AP50 / AP75 the same at one threshold; AR1 / AR10 the
 *   mean final recall over thresholds and categories at that maxDet.  -1.0 when no category counts.
 * ---------------------------------------------------------------------------------------------- */

#ifdef __cplusplus
}
#endif
#endif /* STEMSEG_HIP_H */
