"""The split-staged convolution family (f16x3: the arithmetic of every conv of a default step; bf16x6: what an overflowing clip is re-run in)
against fp64, on every staging and epilogue path -- the split-mode twin of tests/test_gpu_conv_f32.py.

Cases: conv_cases.SPLIT_CASES, each run once per mode it lists -- the f32 file's cases re-planned per mode, plus cases until every
(tile x vec4), (tile x vec_epi), (token x family) and GroupNorm cell is filled (tests/test_conv_plan_host.py prints the matrices and pins every
plan on the CPU; the plan is asserted once more here on the real addresses).  Buffers, poisoning and the double run are those of
tests/test_gpu_conv_f32.py (make_buffers / run_on): output, scratch and guard words are NaN beforehand, the f32 leg and both modes run on the
SAME buffers, weights packed per mode with pack_conv_weight_any.

Reference: fp64 convolution of the same fp32 inputs, epilogue folded in (tests/conv_f32_oracle.py).  Per case and mode:
  (a) the project's split-mode rule, unchanged, over the WHOLE output:  max|split - ref64| <= max(3 max|f32 kernel - ref64|, 4e-7 max|ref64|);
  (b) every output  |dev - ref64| <= (n_acc 2^-23 + c_mode) S + floor -- derived in tests/conv_split_oracle.py (n_acc = 3 K or 6 K products
      + ksplit + 4; c_f16x3 = 3 x 2^-22 (1 + 2^-10): 22 bits per operand and the dropped lo x lo product; c_bf16x6 = 2^-26 (1 + 2^-8): exact split,
      three of nine products dropped; floor, f16x3 only: 2^-33 sum|w| + 2^-37 max|w[co]| sum|x| for terms below fp16's normal range).  The numpy
      restatement of each mode, accumulated in fp32 one product at a time, stays inside it on every case's inputs
      (tests/test_conv_split_cap_host.py);
  (c) pairs that differ in the path only give the SAME BITS, in both modes (reasons: conv_cases.py, above SPLIT_CASES).  The aligned / shifted
      twins of every register-staged tile run on the stress inputs (mixed magnitudes 2^-20 .. 2^17, both zeros, exact rounding ties of the hi
      and of the lo term, values just under 2.6e5): this is the test of split_operand.h's claim that split_pair_f16 equals split_act_f16 bit
      for bit;
  (d) no NaN left, the halo of an interior output exactly zero, a second run gives the same bits, GroupNorm statistics against numpy on the
      device's own output at the f32 file's bounds.
The f32 leg of a case added for the split modes is no case of the f32 file: test_added_cases_f32_leg holds it to that file's bounds (a), (b).

Combinations conv_igemm.hip refuses, absent here: GroupNorm statistics with ReLU or a residual; the decode epilogue on anything but a 1x1 conv
(so "interior" on a 1x1 tile is the decode case); Cin % 4 != 0 and Cout % 32 != 0; flat tiles on an unaligned input, with Cout % 128 != 0, with
GroupNorm statistics or the decode epilogue; block tiles on an unaligned input (Y2Blk: Cout <= 64); flat and block tiles in bf16x6.

Measured on an MI355X: ratio = e_split / max(e_seq, 2^-24 max|ref64|) on the yardstick's positions, e_seq the plain sequential fp32 sum of
tests/conv_f32_oracle.py -- a record, not a bound:

  (ks = ksplit, v4 = vec4, ve = vec_epi as planned; ratios 0.19 .. 1.33 in f16x3 (median 0.69) and 0.22 .. 1.72 in bf16x6 (median 0.82); every pair of (c)
  gave equal bits, and no output passed 0.042 of the cap (b))

  case                           e_seq      | f16x3: tile   ks v4 ve  e_split    ratio | bf16x6: tile  ks v4 ve  e_split    ratio
  k3big_gl_forced                2.159e-06  | Y3Big         1  1  0  1.394e-06  0.646 | Y3Big         1  1  0  2.108e-06  0.976
  k3big_gl_forced_w40            2.380e-06  | Y3Big         1  1  1  1.489e-06  0.625 | Y3Big         1  1  1  1.537e-06  0.646
  k3big_forced_shift             2.159e-06  | Y3Big         1  0  0  1.394e-06  0.646 | Y3Big         1  0  0  2.108e-06  0.976
  k3big_forced_co160             2.068e-06  | Y3Big         1  1  0  1.467e-06  0.709 | Y3Big         1  1  0  1.822e-06  0.881
  k3med_forced                   2.065e-06  | Y3Med         1  1  0  1.625e-06  0.787 | Y3Med         1  1  0  2.045e-06  0.990
  k3small_forced                 6.663e-07  | Y3Small       1  1  0  5.462e-07  0.820 | Y3Small       1  1  0  6.980e-07  1.048
  k3small_forced_w40             8.209e-07  | Y3Small       1  1  1  5.707e-07  0.695 | Y3Small       1  1  1  7.672e-07  0.935
  k3small_dense_unaligned        3.493e-06  | Y3Small       1  0  0  1.620e-06  0.464 | Y3Small       1  0  0  2.278e-06  0.652
  k3med_w40_vec_epilogue         1.992e-06  | Y3Med         1  1  1  1.108e-06  0.556 | Y3Med         1  1  1  1.333e-06  0.669
  k3med_w40_res_from_halo        1.992e-06  | Y3Med         1  1  0  1.108e-06  0.556 | Y3Med         1  1  0  1.333e-06  0.669
  k3med_w40_into_interior        1.963e-06  | Y3Med         1  1  0  1.219e-06  0.621 | Y3Med         1  1  0  1.854e-06  0.944
  k3flatmed                      3.446e-06  | Y3Blk7        1  1  1  2.082e-06  0.604 | Y3Med         1  1  1  3.390e-06  0.984
  k3flatmed_shift                3.446e-06  | Y3Med         1  0  1  2.082e-06  0.604 | Y3Med         1  0  1  3.390e-06  0.984
  k3flatmed56                    3.740e-06  | Y3Small       1  1  0  2.480e-06  0.663 | Y3Small       1  1  0  2.790e-06  0.746
  k3flatmed56_shift              3.740e-06  | Y3Small       1  0  0  2.480e-06  0.663 | Y3Small       1  0  0  2.790e-06  0.746
  k3flatsmall                    1.861e-06  | Y3Small       1  1  0  2.003e-06  1.076 | Y3Small       1  1  0  1.678e-06  0.902
  k3flatsmall_shift              1.861e-06  | Y3Small       1  0  0  2.003e-06  1.076 | Y3Small       1  0  0  1.678e-06  0.902
  k3flatsmall56                  1.759e-06  | Y3Small       1  1  0  1.671e-06  0.950 | Y3Small       1  1  0  1.469e-06  0.835
  k3flatsmall56_shift            1.759e-06  | Y3Small       1  0  0  1.671e-06  0.950 | Y3Small       1  0  0  1.469e-06  0.835
  k3gl_splitk16                  2.570e-06  | Y3Big        16  1  1  4.889e-07  0.190 | Y3Big        16  1  1  5.700e-07  0.222
  k3med_splitk4_by_scratch       1.821e-06  | Y3Med         4  1  1  4.254e-07  0.234 | Y3Med         4  1  1  5.111e-07  0.281
  k3med_splitk_short_last        2.581e-06  | Y3Med         3  1  1  9.304e-07  0.361 | Y3Med         3  1  1  1.147e-06  0.444
  k3small_splitk_scratch_off     2.775e-06  | Y3Small       3  1  0  8.127e-07  0.293 | Y3Small       3  1  0  1.117e-06  0.403
  k3small_splitk2_w37            6.274e-07  | Y3Small       2  1  0  4.191e-07  0.668 | Y3Small       2  1  0  5.601e-07  0.893
  k3flatsmall56_splitk           2.282e-06  | Y3Small       3  1  0  8.091e-07  0.355 | Y3Small       3  1  0  9.561e-07  0.419
  k3flatsmall_splitk             2.735e-06  | Y3Small       3  1  0  1.034e-06  0.378 | Y3Small       3  1  0  1.257e-06  0.460
  k3_gn4_tile                    2.703e-06  | Y3Small       1  1  0  1.252e-06  0.463 | Y3Small       1  1  0  1.785e-06  0.660
  k3_gn8_tile                    1.963e-06  | Y3Med         1  1  1  1.219e-06  0.621 | Y3Med         1  1  1  1.854e-06  0.944
  k3_gn4_splitk                  2.219e-06  | Y3Med         3  1  1  7.970e-07  0.359 | Y3Med         3  1  1  9.376e-07  0.422
  k3_gn8_splitk                  2.993e-06  | Y3Small       3  1  0  7.182e-07  0.240 | Y3Small       3  1  0  1.001e-06  0.334
  k2big_forced                   1.890e-06  | Y2Big         1  1  0  1.300e-06  0.688 | Y2Big         1  1  0  1.828e-06  0.967
  k2med_forced                   1.945e-06  | Y2Med         1  1  0  1.287e-06  0.661 | Y2Med         1  1  0  1.642e-06  0.844
  k2small_forced                 1.720e-06  | Y2Small       1  1  0  1.197e-06  0.696 | Y2Small       1  1  0  1.376e-06  0.800
  k2small_dense_unaligned        1.986e-06  | Y2Small       1  0  0  1.099e-06  0.554 | Y2Small       1  0  0  1.759e-06  0.886
  k2m64                          1.772e-06  | Y2M64         1  1  0  1.112e-06  0.627 | Y2M64         1  1  0  1.571e-06  0.887
  k2m64_co32_w40                 1.519e-06  | Y2M64         1  1  1  1.000e-06  0.658 | Y2M64         1  1  1  1.345e-06  0.885
  k2small_splitk_w37             2.138e-06  | Y2Small       2  1  0  1.450e-06  0.678 | Y2Small       2  1  0  1.647e-06  0.771
  k2m64_splitk_w40               2.724e-06  | Y2M64         2  1  1  1.538e-06  0.565 | Y2M64         3  1  1  1.318e-06  0.484
  k2flatbig                      2.440e-06  | Y2Big         1  1  1  1.623e-06  0.665 | Y2Big         1  1  1  2.125e-06  0.871
  k2flatbig_shift                2.440e-06  | Y2Big         1  0  1  1.623e-06  0.665 | Y2Big         1  0  1  2.125e-06  0.871
  k2flatbig56_splitk2            2.247e-06  | Y2Flat56      1  1  0  1.862e-06  0.829 | Y2Big         2  1  1  1.547e-06  0.688
  k2flatbig56_shift              2.247e-06  | Y2Big         1  0  1  1.862e-06  0.829 | Y2Big         2  0  1  1.547e-06  0.688
  k2flatmed                      1.861e-06  | Y2Small       1  1  0  1.833e-06  0.985 | Y2Small       1  1  0  1.823e-06  0.980
  k2flatmed_shift                1.861e-06  | Y2Small       1  0  0  1.833e-06  0.985 | Y2Small       1  0  0  1.823e-06  0.980
  k2flatmed56                    1.959e-06  | Y2Small       1  1  0  1.349e-06  0.689 | Y2Small       1  1  0  1.605e-06  0.819
  k2flatmed56_shift              1.959e-06  | Y2Small       1  0  0  1.349e-06  0.689 | Y2Small       1  0  0  1.605e-06  0.819
  k2flatmed56_splitk             2.351e-06  | Y2Small       2  1  0  1.170e-06  0.498 | Y2Small       2  1  0  1.900e-06  0.808
  k2_gn8_splitk                  2.708e-06  | Y2Small       2  1  1  1.375e-06  0.508 | Y2Small       2  1  1  1.736e-06  0.641
  k1big_unaligned                8.238e-07  | Y1Big         1  0  0  9.018e-07  1.095 | Y1Big         1  0  0  5.263e-07  0.639
  k1small_unaligned              9.501e-07  | Y1Small       1  0  0  8.814e-07  0.928 | Y1Small       1  0  0  6.603e-07  0.695
  k1small_v5                     5.228e-07  | Y1Small       1  0  0  5.075e-07  0.971 | Y1Small       1  0  0  2.349e-07  0.449
  k1m64_unaligned                7.888e-07  | Y1M64         1  0  0  8.614e-07  1.092 | Y1M64         1  0  0  4.403e-07  0.558
  k1m64_co32_shift               8.292e-07  | Y1M64         1  0  1  7.488e-07  0.903 | Y1M64         1  0  1  4.843e-07  0.584
  k1big_gl                       1.104e-06  | Y1Big         1  1  1  7.035e-07  0.638 | Y1Big         1  1  1  1.139e-06  1.032
  k1big_cin12_falls_to_staged    1.086e-06  | Y1Big         1  1  1  9.635e-07  0.887 | Y1Big         1  1  1  6.091e-07  0.561
  k1big_co160_falls_to_staged    1.339e-06  | Y1Big         1  1  1  1.133e-06  0.846 | Y1Big         1  1  1  1.062e-06  0.793
  k1big_shift_falls_to_staged    1.104e-06  | Y1Big         1  0  1  7.035e-07  0.638 | Y1Big         1  0  1  1.139e-06  1.032
  k1small_gl                     1.406e-06  | Y1Small       1  1  1  7.995e-07  0.569 | Y1Small       1  1  1  9.242e-07  0.658
  k1m64_gl                       1.208e-06  | Y1M64         1  1  1  7.553e-07  0.625 | Y1M64         1  1  1  9.187e-07  0.760
  k1small_decode                 9.582e-07  | Y1Small       1  0  0  7.870e-07  0.821 | Y1Small       1  0  0  6.248e-07  0.652
  k1small_gl_decode              1.455e-06  | Y1Small       1  1  0  9.567e-07  0.658 | Y1Small       1  1  0  9.364e-07  0.644
  k1small_decode_splitk          1.515e-06  | Y1Small       2  0  0  8.626e-07  0.570 | Y1Small       2  0  0  8.873e-07  0.586
  k1small_gl_splitk4             1.468e-06  | Y1Small       2  1  1  7.800e-07  0.531 | Y1Small       2  1  1  6.844e-07  0.466
  k1_gn4_tile                    1.460e-06  | Y1Small       1  1  1  1.048e-06  0.717 | Y1Small       1  1  1  1.000e-06  0.685
  stress_y3big_aligned           1.106e-01  | Y3Big         1  1  1  9.316e-02  0.842 | Y3Big         1  1  1  1.376e-01  1.245
  stress_y3big_shift             1.106e-01  | Y3Big         1  0  1  9.316e-02  0.842 | Y3Big         1  0  1  1.376e-01  1.245
  stress_y3med_aligned           9.624e-02  | Y3Med         1  1  0  7.378e-02  0.767 | Y3Med         1  1  0  1.076e-01  1.118
  stress_y3med_shift             9.624e-02  | Y3Med         1  0  0  7.378e-02  0.767 | Y3Med         1  0  0  1.076e-01  1.118
  stress_y3small_aligned         4.008e-02  | Y3Small       1  1  1  3.656e-02  0.912 | Y3Small       1  1  1  3.493e-02  0.872
  stress_y3small_shift           4.008e-02  | Y3Small       1  0  1  3.656e-02  0.912 | Y3Small       1  0  1  3.493e-02  0.872
  stress_y2big_aligned           1.763e-01  | Y2Big         1  1  0  1.089e-01  0.618 | Y2Big         1  1  0  1.215e-01  0.689
  stress_y2big_shift             1.763e-01  | Y2Big         1  0  0  1.089e-01  0.618 | Y2Big         1  0  0  1.215e-01  0.689
  stress_y2med_aligned           1.522e-01  | Y2Med         1  1  1  1.072e-01  0.704 | Y2Med         1  1  1  1.203e-01  0.790
  stress_y2med_shift             1.522e-01  | Y2Med         1  0  1  1.072e-01  0.704 | Y2Med         1  0  1  1.203e-01  0.790
  stress_y2small_aligned         1.059e-01  | Y2Small       1  1  1  8.199e-02  0.774 | Y2Small       1  1  1  9.266e-02  0.875
  stress_y2small_shift           1.059e-01  | Y2Small       1  0  1  8.199e-02  0.774 | Y2Small       1  0  1  9.266e-02  0.875
  stress_y2m64_aligned           1.024e-01  | Y2M64         1  1  0  1.363e-01  1.331 | Y2M64         1  1  0  1.762e-01  1.721
  stress_y2m64_shift             1.024e-01  | Y2M64         1  0  0  1.363e-01  1.331 | Y2M64         1  0  0  1.762e-01  1.721
  stress_y1big_aligned           8.000e-02  | Y1Big         1  1  1  6.701e-02  0.838 | Y1Big         1  1  1  8.438e-02  1.055
  stress_y1big_shift             8.000e-02  | Y1Big         1  0  1  6.701e-02  0.838 | Y1Big         1  0  1  8.438e-02  1.055
  stress_y1small_aligned         8.009e-02  | Y1Small       1  1  1  6.466e-02  0.807 | Y1Small       1  1  1  9.475e-02  1.183
  stress_y1small_shift           8.009e-02  | Y1Small       1  0  1  6.466e-02  0.807 | Y1Small       1  0  1  9.475e-02  1.183
  stress_y1m64_aligned           6.236e-02  | Y1M64         1  1  1  4.898e-02  0.785 | Y1M64         1  1  1  6.249e-02  1.002
  stress_y1m64_shift             6.236e-02  | Y1M64         1  0  1  4.898e-02  0.785 | Y1M64         1  0  1  6.249e-02  1.002
  stress_y1wide_aligned          1.106e-01  | Y1Wide        1  1  1  8.591e-02  0.777 | Y1Wide        1  1  1  8.013e-02  0.725
  stress_y1wide_shift            1.106e-01  | Y1Wide        1  0  1  8.591e-02  0.777 | Y1Wide        1  0  1  8.013e-02  0.725
  y3med_wide_rows                2.589e-06  | Y3Med         1  1  0  1.473e-06  0.569 | Y3Med         1  1  0  2.322e-06  0.897
  y2big_wide_rows                3.681e-06  | Y2Big         1  1  1  2.547e-06  0.692 | Y2Big         1  1  1  3.785e-06  1.028
  y3big_dense                    2.720e-06  | Y3Big         1  0  0  1.632e-06  0.600 | Y3Big         1  0  0  2.678e-06  0.985
  y3med_dense                    3.577e-06  | Y3Med         1  0  0  1.834e-06  0.513 | Y3Med         1  0  0  2.706e-06  0.757
  y2big_dense                    2.578e-06  | Y2Big         1  0  0  1.469e-06  0.570 | Y2Big         1  0  0  2.033e-06  0.789
  y2med_dense                    2.344e-06  | Y2Med         1  0  0  1.908e-06  0.814 | Y2Med         1  0  0  2.578e-06  1.100
  y2m64_dense                    1.299e-06  | Y2M64         1  0  0  1.250e-06  0.962 | Y2M64         1  0  0  1.023e-06  0.787
  y2med_w40_vec_epilogue         1.587e-06  | Y2Med         1  1  1  1.226e-06  0.772 | Y2Med         1  1  1  2.146e-06  1.352
  y2small_w40_into_interior      1.541e-06  | Y2Small       1  1  0  1.190e-06  0.772 | Y2Small       1  1  0  1.264e-06  0.820
  y1wide_v1001                   1.683e-06  | Y1Wide        1  0  0  1.056e-06  0.627 | Y1Wide        1  0  0  1.422e-06  0.845
  y1wide_v5                      3.492e-07  | Y1Wide        1  0  0  3.736e-07  1.070 | Y1Wide        1  0  0  2.782e-07  0.797
  y1wide_decode                  1.297e-06  | Y1Wide        1  0  0  8.688e-07  0.670 | Y1Wide        1  0  0  8.336e-07  0.643
  y1big_decode_splitk            1.604e-06  | Y1Big         2  1  1  9.263e-07  0.577 | Y1Big         2  1  1  9.643e-07  0.601
  k2_gn4_tile                    1.711e-06  | Y2Small       1  1  0  1.730e-06  1.011 | Y2Small       1  1  0  1.728e-06  1.010
  k2_gn8_tile                    1.926e-06  | Y2M64         1  1  1  1.454e-06  0.755 | Y2M64         1  1  1  1.753e-06  0.910
  k2_gn4_splitk                  3.652e-06  | Y2Small       2  1  0  1.546e-06  0.423 | Y2Small       3  1  0  1.314e-06  0.360
  k1_gn8_tile                    1.243e-06  | Y1M64         1  0  0  7.897e-07  0.635 | Y1M64         1  0  0  1.170e-06  0.941
  k1_gn4_splitk                  1.783e-06  | Y1Small       2  1  1  8.684e-07  0.487 | Y1Small       2  1  1  1.044e-06  0.585
  k1_gn8_splitk                  1.620e-06  | Y1Small       2  0  0  8.522e-07  0.526 | Y1Small       2  0  0  1.099e-06  0.678
  y2flat56                       1.959e-06  | Y2Flat56      1  1  0  1.349e-06  0.689 | -             -  -  -  -          -
  y2flat56_as_2d                 1.959e-06  | Y2Big         1  1  0  1.349e-06  0.689 | Y2Big         1  1  0  1.605e-06  0.819
  y2flat112                      2.704e-06  | Y2Flat112     1  1  0  1.714e-06  0.634 | -             -  -  -  -          -
  y2flat112_as_2d                2.704e-06  | Y2Big         1  1  0  1.714e-06  0.634 | Y2Big         1  1  0  1.872e-06  0.693
  y2flat224                      1.802e-06  | Y2Flat224     1  1  0  1.380e-06  0.766 | -             -  -  -  -          -
  y2flat224_as_2d                1.802e-06  | Y2Big         1  1  1  1.380e-06  0.766 | Y2Big         1  1  1  1.685e-06  0.935
  y2flat56_splitk                3.349e-06  | Y2Flat56      2  1  0  1.502e-06  0.449 | -             -  -  -  -          -
  y3blk                          2.143e-06  | Y3Blk         1  1  0  1.408e-06  0.657 | -             -  -  -  -          -
  y3blk_as_2d                    2.143e-06  | Y3Big         1  1  0  1.408e-06  0.657 | Y3Big         1  1  0  1.831e-06  0.854
  y3blk_gn8                      2.388e-06  | Y3Blk         1  1  0  1.952e-06  0.817 | -             -  -  -  -          -
  y3blk_splitk                   1.203e-06  | Y3Blk         3  1  1  5.369e-07  0.446 | -             -  -  -  -          -
  y2blk                          2.287e-06  | Y2Blk         1  1  0  1.816e-06  0.794 | -             -  -  -  -          -
  y2blk_as_2d                    2.287e-06  | Y2Big         1  1  0  1.816e-06  0.794 | Y2Big         1  1  0  2.012e-06  0.880
  y2blk_res                      3.195e-06  | Y2Blk         1  1  1  2.735e-06  0.856 | -             -  -  -  -          -
  y3blk7                         2.071e-06  | Y3Blk7        1  1  1  2.007e-06  0.969 | -             -  -  -  -          -
  y3blk7_as_2d                   2.071e-06  | Y3Med         1  1  1  2.007e-06  0.969 | Y3Med         1  1  1  1.611e-06  0.778
  y3blk7_into_interior           1.620e-06  | Y3Blk7        1  1  0  1.501e-06  0.926 | -             -  -  -  -          -
"""
import numpy as np
import pytest

from tests import conv_cases as cc
from tests import conv_f32_oracle as oracle
from tests import conv_split_oracle as so
from tests.test_gpu_conv_f32 import FACTOR, make_buffers, run_on

pytestmark = pytest.mark.gpu

_CASE = {}
_PAIRED = set(s.case.name for s in cc.SPLIT_CASES if s.case.pair) | set(s.case.pair for s in cc.SPLIT_CASES if s.case.pair)


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def _gn_ok(case, r):
    groups = cc.gn_groups(case)
    if not groups:
        return True, ""
    st = r["stats"][0].reshape(groups, 2)
    o = r["out"].astype(np.float64).reshape(groups, -1)
    mean, rstd = o.mean(1), 1.0 / np.sqrt(o.var(1) + 1e-5)
    e_mean, e_rstd = float(np.abs(st[:, 0] - mean).max()), float(np.abs(st[:, 1] - rstd).max())
    ok = np.array_equal(r["stats"][0], r["stats"][1]) and e_mean <= 2e-6 * max(1.0, np.abs(mean).max()) and e_rstd <= 1e-4 * rstd.max()
    return ok, "GroupNorm statistics: mean off by %.3g, rstd by %.3g (or another run, other bits)" % (e_mean, e_rstd)


def _summary(case, d, r, prec, ksplit):
    """What the assertions need of one run, without the second output."""
    out, ref = r["out"], d["ref"]
    err = np.abs(out.astype(np.float64) - ref)
    bound = so.cap(case, prec, ksplit) if prec != "f32" else (d["K"] + ksplit + 4) * 2.0 ** -23 * d["S"]
    finite = bool(np.isfinite(out).all())
    (t, y, x), _, e_seq = oracle.yardstick(case, ())
    gn_ok, gn_msg = _gn_ok(case, r)
    return dict(recs=r["recs"], finite=finite, n_bad=int((~np.isfinite(out)).sum()), halo_clean=r["halo_clean"],
                same_bits=bool(np.array_equal(out.view(np.uint32), r["out2"].view(np.uint32))), e_all=float(err.max()) if finite else float("inf"),
                e_sub=float(err[:, t, y, x].max()) if finite else float("inf"), e_seq=e_seq, ref_max=float(np.abs(ref).max()),
                over_cap=int((~(err <= bound)).sum()), worst_cap=float(np.nanmax(err / (bound + 1e-300))), gn_ok=gn_ok, gn_msg=gn_msg,
                out=out if case.name in _PAIRED else None)


def case_results(hip, name):
    """f32 leg and every listed mode of a case on the same buffers, once."""
    if name not in _CASE:
        sc = cc.SPLIT_BY_NAME[name]
        case = sc.case
        d = oracle.reference(case)
        bufs = make_buffers(case, d)
        res = {}
        for prec in ("f32",) + tuple(m for m in cc.SPLIT_MODES if m in sc.want):
            r = run_on(hip, case, d, bufs, prec)
            res[prec] = _summary(case, d, r, prec, max(q["ksplit"] for q in r["recs"]))
        res["f32"]["out"] = None
        _CASE[name] = res
    return _CASE[name]


@pytest.mark.parametrize("name,prec", cc.SPLIT_RUNS)
def test_split_conv_vs_fp64(hip, name, prec):
    sc = cc.SPLIT_BY_NAME[name]
    case, want = sc.case, sc.want[prec]
    res = case_results(hip, name)
    s, f = res[prec], res["f32"]
    # the path: what tests/test_conv_plan_host.py pins on made-up addresses holds on the real ones
    (q,) = s["recs"]
    assert cc.Want(cc.tile_name(q), q["vec4"], q["vec_epi"], q["ksplit"], q["reduce"]) == want and q["precision"] == prec
    unit = max(s["e_seq"], 2.0 ** -24 * s["ref_max"])
    print("RATIO %-30s %-6s %-10s ksplit %2d vec4 %d vec_epi %d  e_seq %.3e  e_f32 %.3e  e_split %.3e  ratio %.3f   (all outputs: e_split %.3e, e_f32 %.3e, "
          "max err/cap(b) %.4f)" % (name, prec, want.tile, want.ksplit, want.vec4, want.vec_epi, s["e_seq"], f["e_sub"], s["e_sub"], s["e_sub"] / unit,
                                    s["e_all"], f["e_all"], s["worst_cap"]))
    # (d) no stray values
    assert s["finite"], "%d outputs are not finite" % s["n_bad"]
    assert s["halo_clean"], "the halo of the output volume was written"
    assert s["same_bits"], "a second run gives other bits"
    assert s["gn_ok"], s["gn_msg"]
    # (a) the split-mode rule, whole output, against the f32 kernel on the same buffers
    assert f["finite"]
    allowed = max(3.0 * f["e_all"], 4e-7 * s["ref_max"])
    assert s["e_all"] <= allowed, "(a) %.3e > max(3 x %.3e, 4e-7 x %.3e)" % (s["e_all"], f["e_all"], s["ref_max"])
    # (b) the derived cap, every output
    assert s["over_cap"] == 0, "(b) %d outputs beyond the cap, worst %.3g x" % (s["over_cap"], s["worst_cap"])


@pytest.mark.parametrize("name", [s.case.name for s in cc.SPLIT_CASES if s.case.name not in cc.CASES_BY_NAME])
def test_added_cases_f32_leg(hip, name):
    """The yardstick leg of rule (a) is itself held to fp64 where tests/test_gpu_conv_f32.py has no such case: its bounds (a), (b) and (d)."""
    f = case_results(hip, name)["f32"]
    assert f["finite"] and f["halo_clean"] and f["same_bits"] and f["gn_ok"], f["gn_msg"]
    assert f["e_sub"] <= FACTOR * max(f["e_seq"], 2.0 ** -24 * f["ref_max"])
    assert f["over_cap"] == 0, "%d outputs beyond (K + ksplit + 4) 2^-23 S, worst %.3g x" % (f["over_cap"], f["worst_cap"])


@pytest.mark.parametrize("name,prec", [(n, m) for n, m in cc.SPLIT_RUNS if cc.SPLIT_BY_NAME[n].case.pair and m in cc.SPLIT_BY_NAME[cc.SPLIT_BY_NAME[n].case.pair].want])
def test_split_paths_agree(hip, name, prec):
    """(c): the same convolution through two paths, in one mode."""
    case = cc.SPLIT_BY_NAME[name].case
    a, b = case_results(hip, name), case_results(hip, case.pair)
    oa, ob = a[prec]["out"], b[prec]["out"]
    diff = float(np.abs(oa.astype(np.float64) - ob).max())
    n_diff = int((oa.view(np.uint32) != ob.view(np.uint32)).sum())
    print("PAIR %-30s %-6s %-10s vs %-30s %-10s max|diff| %.3e, differing elements %d of %d"
          % (name, prec, cc.SPLIT_BY_NAME[name].want[prec].tile, case.pair, cc.SPLIT_BY_NAME[case.pair].want[prec].tile, diff, n_diff, oa.size))
    assert diff <= max(3.0 * a["f32"]["e_all"], 4e-7 * a[prec]["ref_max"])
    assert case.bits and n_diff == 0, "same k order and the same split arithmetic by construction: the two paths must give the same bits"
