"""The convolution family's case list and launch-plan helpers, shared by tests/test_conv_plan_host.py (which tile, split and row cut
every case exercises: checked on the CPU through ``hip.conv3d_plan``), tests/test_gpu_conv_f32.py (the same cases against fp64) and
tests/test_gpu_conv_split.py (SPLIT_CASES, at the end: the split modes' own matrix against fp64).

A case names the tile instantiation it exists for; the host test fails when ``launch_conv3d`` stops choosing it.  Nothing here needs a
GPU: volumes are described by their geometry (offset of the view in its buffer, strides, extents, buffer size) and the plan is asked
with a made-up base address of the same alignment the device buffers have."""
import collections

# ---------------------------------------------------------------------------------------------------------------- tiles
# identity of a tile as conv3d_plan reports it: (kt, kh, kw, ck, mt, rows, tw, nt, pmax, gl, blk)
Tile = collections.namedtuple("Tile", "kt kh kw ck mt rows tw nt pmax gl blk")
# the fp32-input instantiations of conv_igemm.hip, written out (test_conv_plan_host.py counts the `using ... = ConvCfg<` lines against this)
F32_TILES = {
    "K3Big": Tile(3, 3, 3, 4, 128, 8, 32, 256, 0, 0, 0),
    "K3BigGL": Tile(3, 3, 3, 2, 128, 8, 32, 256, 0, 1, 0),
    "K3Med": Tile(3, 3, 3, 4, 128, 4, 32, 128, 0, 0, 0),
    "K3Small": Tile(3, 3, 3, 4, 128, 2, 32, 64, 0, 0, 0),
    "K1Big": Tile(1, 1, 1, 32, 128, 1, 256, 256, 0, 0, 0),
    "K1Small": Tile(1, 1, 1, 32, 128, 1, 128, 128, 0, 0, 0),
    "K1M64": Tile(1, 1, 1, 32, 64, 1, 256, 256, 0, 0, 0),
    "K1BigGL": Tile(1, 1, 1, 16, 128, 1, 256, 256, 0, 1, 0),
    "K1SmallGL": Tile(1, 1, 1, 16, 128, 1, 128, 128, 0, 1, 0),
    "K1M64GL": Tile(1, 1, 1, 16, 64, 1, 256, 256, 0, 1, 0),
    "K2Big": Tile(1, 3, 3, 8, 128, 8, 32, 256, 0, 0, 0),
    "K2Med": Tile(1, 3, 3, 8, 128, 4, 32, 128, 0, 0, 0),
    "K2Small": Tile(1, 3, 3, 8, 128, 2, 32, 64, 0, 0, 0),
    "K2M64": Tile(1, 3, 3, 8, 64, 8, 32, 256, 0, 0, 0),
    "K2FlatBig": Tile(1, 3, 3, 8, 128, 1, 256, 256, 112, 0, 0),
    "K2FlatMed": Tile(1, 3, 3, 8, 128, 1, 128, 128, 112, 0, 0),
    "K3FlatMed": Tile(3, 3, 3, 4, 128, 1, 128, 128, 112, 0, 0),
    "K3FlatSmall": Tile(3, 3, 3, 4, 128, 1, 64, 64, 112, 0, 0),
    "K2FlatBig56": Tile(1, 3, 3, 8, 128, 1, 256, 256, 56, 0, 0),
    "K2FlatMed56": Tile(1, 3, 3, 8, 128, 1, 128, 128, 56, 0, 0),
    "K3FlatMed56": Tile(3, 3, 3, 4, 128, 1, 128, 128, 56, 0, 0),
    "K3FlatSmall56": Tile(3, 3, 3, 4, 128, 1, 64, 64, 56, 0, 0),
}


def split_tiles(prec):
    """SplitTiles<BFV> of conv_split_family.h: the 1x3x3 chunk is 16 channels in f16x3 and 8 in bf16x6 (split_chunk_channels)."""
    ck2 = 16 if prec == "f16x3" else 8
    return {
        "Y3Big": Tile(3, 3, 3, 4, 128, 16, 32, 512, 0, 0, 0),
        "Y3Med": Tile(3, 3, 3, 4, 128, 8, 32, 256, 0, 0, 0),
        "Y3Small": Tile(3, 3, 3, 4, 128, 4, 32, 128, 0, 0, 0),
        "Y2Big": Tile(1, 3, 3, ck2, 128, 16, 32, 512, 0, 0, 0),
        "Y2Med": Tile(1, 3, 3, ck2, 128, 4, 32, 128, 0, 0, 0),
        "Y2Small": Tile(1, 3, 3, ck2, 128, 2, 32, 64, 0, 0, 0),
        "Y2M64": Tile(1, 3, 3, ck2, 64, 8, 32, 256, 0, 0, 0),
        "Y1Big": Tile(1, 1, 1, 32, 128, 1, 256, 256, 0, 0, 0),
        "Y1Small": Tile(1, 1, 1, 32, 128, 1, 128, 128, 0, 0, 0),
        "Y1M64": Tile(1, 1, 1, 32, 64, 1, 256, 256, 0, 0, 0),
        "Y1Wide": Tile(1, 1, 1, 32, 256, 1, 256, 256, 0, 0, 0),
        "Y2Flat56": Tile(1, 3, 3, ck2, 128, 1, 512, 512, 56, 0, 0),
        "Y2Flat112": Tile(1, 3, 3, ck2, 128, 1, 512, 512, 112, 0, 0),
        "Y2Flat224": Tile(1, 3, 3, ck2, 128, 1, 512, 512, 224, 0, 0),
        "Y4Stem": Tile(1, 4, 4, 16, 64, 16, 32, 512, 0, 0, 0),
        "Y3Blk": Tile(3, 3, 3, 4, 128, 20, 24, 512, 0, 0, 5),
        "Y2Blk": Tile(1, 3, 3, ck2, 128, 20, 24, 512, 0, 0, 5),
        "Y3Blk7": Tile(3, 3, 3, 4, 128, 4, 56, 256, 0, 0, 1),
    }


# what launch_split_family can return per mode (Y4Stem aside: launch_stem_f16x3, its own fp64 tests in tests/test_gpu_parity.py).  The flat and
# block forms are f16x3 only (`if constexpr (BFV == 3)`).
SPLIT_REACHABLE = {
    "bf16x6": ("Y3Big", "Y3Med", "Y3Small", "Y2Big", "Y2Med", "Y2Small", "Y2M64", "Y1Big", "Y1Small", "Y1M64", "Y1Wide"),
    "f16x3": ("Y3Big", "Y3Med", "Y3Small", "Y2Big", "Y2Med", "Y2Small", "Y2M64", "Y1Big", "Y1Small", "Y1M64", "Y1Wide", "Y2Flat56", "Y2Flat112",
              "Y2Flat224", "Y3Blk", "Y2Blk", "Y3Blk7"),          # (f16x3 takes Y1Big only when tile_cfg 1 forces it: its own 1x1 choice is `cfg = 2`)
}


def tile_name(rec):
    """Name of the instantiation a plan record describes."""
    ident = Tile(*(rec[f] for f in Tile._fields))
    table = F32_TILES if rec["precision"] == "f32" else split_tiles(rec["precision"])
    names = [n for n, t in table.items() if t == ident]
    assert len(names) == 1, (rec, names)
    return names[0]


# ---------------------------------------------------------------------------------------------------------------- geometry
Geom = collections.namedtuple("Geom", "offset cs ts ys C T H W total")      # a view: floats from the buffer base, strides, extents, buffer floats
TAPS = {"k3": (3, 3, 3), "k2": (1, 3, 3), "k1": (1, 1, 1)}


def _round4(n):
    return (n + 3) // 4 * 4


def halo_geom(kind, C, T, H, W, shift=0):
    """The zero-haloed volume a (kt, 3, 3) convolution reads (the whole haloed view), or with shift = -1 its INTERIOR (what a producer writes)."""
    pitch = _round4(W + 2)
    ts = (H + 2) * pitch
    Tp = T + 2 if kind == "k3" else T
    cs = Tp * ts
    total = C * cs + 64 + 4
    if shift < 0:
        return Geom((ts if kind == "k3" else 0) + pitch + 1, cs, ts, pitch, C, T, H, W, total)
    return Geom(shift, cs, ts, pitch, C, Tp, H + 2, W + 2, total)


def dense_geom(C, T, H, W, shift=0):
    return Geom(shift, T * H * W, H * W, W, C, T, H, W, C * T * H * W + 4)


def flat_geom(C, V, shift=0):
    return Geom(shift, V, 0, 0, C, 1, 1, V, C * V + 4)


# ---------------------------------------------------------------------------------------------------------------- cases
# kind: k3 / k2 / k1 (k1: V = T * H * W voxels on the flat [C][V] view; "decode" in the epilogue stores them into a [T][H][W] volume)
# cfg: tile_cfg; scratch: split-K scratch in floats (0: none); scratch_off: 1 = the scratch pointer sits one float off a 16-byte boundary
# inp:  "halo"  zero-haloed, 16-byte aligned rows (k1: the aligned flat view)
#       "dense" an un-haloed dense [C][T + kt - 1][H + 2][W + 2] volume (every value random), rows not 16-byte aligned
#       "shift" the zero-haloed volume, its base one float off a 16-byte boundary
# out:  "dense" | "interior" (the interior of a zero-haloed volume whose halo must stay zero)
# epi:  "+"-joined: nobias, relu, res (dense residual), reshalo (residual read through strides from the interior of a zero-haloed volume), decode,
#       gn4 / gn8 (stemseg_hip_conv3d_gn with groups of 4 / 8 channels)
# tile: the instantiation the case exists for; ksplit: the split-K factor it must plan (1: none); cut: a planned row cut (two launches)
# reduce: the form of the split-K reduce ("vec16" | "scalar" | None); pair: name of the case it differs from in the path only, and
# bits: whether the pair's outputs must be bit-identical (same k order per output by construction -- see the reason next to the case)
Case = collections.namedtuple("Case", "name kind Cin Cout T H W cfg scratch inp out epi tile ksplit cut reduce scratch_off pair bits factor")


def C(name, kind, Cin, Cout, T, H, W, tile, cfg=0, scratch=0, inp="halo", out="dense", epi="", ksplit=1, cut=False, reduce=None, scratch_off=0,
      pair=None, bits=False, factor=3.0):
    return Case(name, kind, Cin, Cout, T, H, W, cfg, scratch, inp, out, epi, tile, ksplit, cut, reduce, scratch_off, pair, bits, factor)


def epi_set(case):
    return set(t for t in case.epi.split("+") if t)


def in_geom(case):
    kt = TAPS[case.kind][0]
    if case.kind == "k1":
        return flat_geom(case.Cin, case.T * case.H * case.W, 0 if case.inp == "halo" else 1)
    if case.inp == "dense":
        return dense_geom(case.Cin, case.T + kt - 1, case.H + 2, case.W + 2)
    return halo_geom(case.kind, case.Cin, case.T, case.H, case.W, 1 if case.inp == "shift" else 0)


def out_geom(case):
    if case.kind == "k1" and "decode" not in epi_set(case):
        assert case.out == "dense"
        return flat_geom(case.Cout, case.T * case.H * case.W)
    if case.out == "interior":
        return halo_geom("k3" if case.kind == "k3" else "k2", case.Cout, case.T, case.H, case.W, -1)
    return dense_geom(case.Cout, case.T, case.H, case.W)


def res_geom(case):
    """Geometry of the residual (addressed at the output's (c, t, y, x)), or None."""
    e = epi_set(case)
    if "reshalo" in e:
        return halo_geom("k3" if case.kind == "k3" else "k2", case.Cout, case.T, case.H, case.W, -1)
    if "res" in e:
        return dense_geom(case.Cout, case.T, case.H, case.W)
    return None


def gn_groups(case):
    e = epi_set(case)
    return case.Cout // 4 if "gn4" in e else (case.Cout // 8 if "gn8" in e else 0)


BASE = 1 << 32          # made-up device address of a buffer (torch's allocations are 512-byte aligned: so is this)


def volume(hip, g, base):
    return hip.Volume(base + 4 * g.offset, g.cs, g.ts, g.ys, g.C, g.T, g.H, g.W, g.total - g.offset)


def plan(hip, case, precision="f32", bases=None, zero_t_halo=False):
    """conv3d_plan of the case.  bases: (input, output, residual, scratch) buffer addresses -- made up unless the GPU test passes its real ones."""
    b_in, b_out, b_res, b_scr = bases or (BASE, 2 * BASE, 3 * BASE, 4 * BASE)
    e = epi_set(case)
    epi = dict(precision=precision, relu=int("relu" in e))
    rg = res_geom(case)
    if rg is not None:
        epi.update(residual=b_res + 4 * rg.offset, res_strides=(rg.cs, rg.ts, rg.ys))
    if "decode" in e:
        epi.update(decode=(case.H, case.W))
    return hip.conv3d_plan(volume(hip, in_geom(case), b_in), volume(hip, out_geom(case), b_out), TAPS[case.kind], case.cfg,
                           (b_scr + 4 * case.scratch_off, case.scratch) if case.scratch else None, epi, bias=0 if "nobias" in e else 1 << 20,
                           gn_groups=gn_groups(case), zero_t_halo=zero_t_halo)


def signature(rec):
    """What ties a yardstick leg to a checked case: the instantiation, split-K or not, 16-byte staging and 16-byte epilogue as launched."""
    return (tile_name(rec), rec["ksplit"] > 1, rec["vec4"], rec["vec_epi"])


def describe(rec):
    return "%-13s ksplit %2d (%d of %2d chunks each) grid %-14s rows [%d, %d) vec4 %d vec_epi %d reduce %-6s gn %s" % (
        tile_name(rec), rec["ksplit"], rec["chunks_per_split"], rec["nchunks"], rec["grid"], rec["row0"], rec["row1"], rec["vec4"], rec["vec_epi"],
        rec["reduce"], rec["gn"])


def _s16(Cout, T, H, W):
    return 16 * Cout * T * H * W          # scratch for the largest split: 16 slabs


CASES = [
    # ---- 3x3x3, 2-D tiles --------------------------------------------------------------------------------------------------------------------
    # The big tile, forced: GL (aligned input, Cout % 128 == 0) and its register-staged form (Cout 160; the same shape on rows one float off).
    # K3BigGL walks 2-channel chunks and K3Big 4-channel ones: the pair is held to (a), not to equal bits (ConvCfg CK 2 against 4).
    C("k3big_gl_forced", "k3", 12, 128, 2, 11, 37, "K3BigGL", cfg=1),
    C("k3big_gl_forced_w40", "k3", 12, 128, 2, 11, 40, "K3BigGL", cfg=1, epi="relu+res"),            # (W % 4 == 0: the 16-byte epilogue)
    C("k3big_forced_shift", "k3", 12, 128, 2, 11, 37, "K3Big", cfg=1, inp="shift", pair="k3big_gl_forced"),
    C("k3big_forced_co160", "k3", 12, 160, 2, 11, 37, "K3Big", cfg=1, epi="relu"),
    C("k3med_forced", "k3", 12, 160, 2, 9, 37, "K3Med", cfg=2, epi="nobias"),
    C("k3small_forced", "k3", 12, 32, 1, 5, 35, "K3Small", cfg=3, epi="relu+res"),
    C("k3small_forced_w40", "k3", 12, 32, 1, 5, 40, "K3Small", cfg=3),
    C("k3small_dense_unaligned", "k3", 16, 64, 2, 7, 13, "K3Small", inp="dense"),
    C("k3med_w40_vec_epilogue", "k3", 12, 128, 2, 9, 40, "K3Med", cfg=2, epi="relu+res"),              # W % 4 == 0: 16-byte epilogue ...
    C("k3med_w40_res_from_halo", "k3", 12, 128, 2, 9, 40, "K3Med", cfg=2, epi="relu+reshalo"),          # ... turned off by a misaligned residual
    C("k3med_w40_into_interior", "k3", 12, 128, 2, 9, 40, "K3Med", cfg=2, out="interior"),
    # launch_planned on >= 512 workgroups of the big tile: no scratch (one plain launch), and with scratch the row cut of launch_rows -- whole
    # rows + split-K rows; the GPU test puts yardstick positions on both sides of the seam
    C("k3gl_planned", "k3", 12, 128, 8, 61, 250, "K3BigGL"),
    C("k3gl_planned_row_cut", "k3", 12, 128, 4, 150, 250, "K3BigGL", scratch=_s16(128, 4, 150, 250), ksplit=3, cut=True, reduce="scalar"),
    C("k3big_planned_row_cut", "k3", 12, 160, 4, 77, 250, "K3Big", scratch=_s16(160, 4, 77, 250), ksplit=3, cut=True, reduce="scalar"),
    C("k3med_planned_row_cut", "k3", 12, 160, 3, 101, 250, "K3Med", scratch=_s16(160, 3, 101, 250), ksplit=2, cut=True, reduce="scalar"),
    # ---- 3x3x3, flat tiles (auto only), each with the same shape one float off: the flat form is refused and the 2-D tile must agree within (a)
    C("k3flatmed", "k3", 12, 128, 8, 60, 108, "K3FlatMed"),
    C("k3flatmed_shift", "k3", 12, 128, 8, 60, 108, "K3Med", inp="shift", pair="k3flatmed", bits=True),
    C("k3flatmed56", "k3", 12, 128, 8, 94, 50, "K3FlatMed56", epi="relu+res"),
    C("k3flatmed56_shift", "k3", 12, 128, 8, 94, 50, "K3Med", inp="shift", epi="relu+res", pair="k3flatmed56", bits=True),
    C("k3flatsmall", "k3", 12, 160, 2, 9, 70, "K3FlatSmall", epi="nobias"),
    C("k3flatsmall_shift", "k3", 12, 160, 2, 9, 70, "K3Small", inp="shift", epi="nobias", pair="k3flatsmall", bits=True),
    C("k3flatsmall56", "k3", 12, 128, 2, 9, 37, "K3FlatSmall56", epi="relu+reshalo", out="interior"),
    C("k3flatsmall56_shift", "k3", 12, 128, 2, 9, 37, "K3Small", inp="shift", epi="relu+reshalo", out="interior", pair="k3flatsmall56", bits=True),
    # ---- 3x3x3, split-K: 16, 4 and 2 ways, a short last split (5 chunks in splits of 2 + 2 + 1; capped by ksplit * 2 <= nchunks), both reduce forms
    C("k3gl_splitk16", "k3", 64, 128, 1, 6, 40, "K3BigGL", cfg=1, scratch=_s16(128, 1, 6, 40), ksplit=16, reduce="vec16", epi="relu+res"),
    C("k3med_splitk4_by_scratch", "k3", 32, 128, 1, 6, 40, "K3Med", cfg=2, scratch=4 * 128 * 6 * 40, ksplit=4, reduce="vec16"),
    C("k3med_splitk_short_last", "k3", 20, 128, 2, 5, 40, "K3Med", cfg=2, scratch=_s16(128, 2, 5, 40), ksplit=3, reduce="vec16", epi="nobias"),
    C("k3small_splitk_scratch_off", "k3", 20, 128, 2, 5, 40, "K3Small", cfg=3, scratch=_s16(128, 2, 5, 40), scratch_off=1, ksplit=3, reduce="scalar",
      epi="relu+res"),
    C("k3small_splitk2_w37", "k3", 16, 32, 1, 5, 37, "K3Small", cfg=3, scratch=2 * 32 * 5 * 37, ksplit=2, reduce="scalar", epi="relu+reshalo"),
    C("k3flatsmall56_splitk", "k3", 20, 128, 2, 9, 37, "K3FlatSmall56", scratch=_s16(128, 2, 9, 37), ksplit=3, reduce="scalar", epi="relu+res"),
    C("k3flatsmall_splitk", "k3", 20, 128, 2, 9, 70, "K3FlatSmall", scratch=_s16(128, 2, 9, 70), ksplit=3, reduce="scalar", out="interior"),
    # ---- GroupNorm statistics in the epilogue (stemseg_hip_conv3d_gn), groups of 4 and 8 channels, per tile and in the split-K reduce
    C("k3_gn4_tile", "k3", 12, 64, 2, 9, 37, "K3FlatSmall56", epi="gn4"),
    C("k3_gn8_tile", "k3", 12, 128, 2, 9, 40, "K3Med", cfg=2, epi="gn8"),
    C("k3_gn4_splitk", "k3", 20, 128, 2, 5, 40, "K3Med", cfg=2, scratch=_s16(128, 2, 5, 40), ksplit=3, reduce="vec16", epi="gn4"),
    C("k3_gn8_splitk", "k3", 20, 64, 2, 9, 37, "K3Small", cfg=3, scratch=_s16(64, 2, 9, 37), ksplit=3, reduce="scalar", epi="gn8"),
    # ---- 1x3x3 ----------------------------------------------------------------------------------------------------------------------------------
    C("k2big_forced", "k2", 12, 160, 2, 11, 37, "K2Big", cfg=1, epi="relu+res"),
    C("k2med_forced", "k2", 12, 160, 2, 11, 37, "K2Med", cfg=2, epi="nobias"),
    C("k2small_forced", "k2", 12, 160, 2, 11, 37, "K2Small", cfg=3, epi="relu"),
    C("k2small_dense_unaligned", "k2", 12, 128, 2, 7, 13, "K2Small", inp="dense"),
    C("k2m64", "k2", 12, 64, 2, 11, 37, "K2M64", epi="relu+reshalo", out="interior"),
    C("k2m64_co32_w40", "k2", 12, 32, 2, 11, 40, "K2M64", epi="relu+res"),
    C("k2small_splitk_w37", "k2", 20, 128, 2, 11, 37, "K2Small", cfg=3, scratch=_s16(128, 2, 11, 37), ksplit=2, reduce="scalar", epi="relu+res"),
    C("k2m64_splitk_w40", "k2", 36, 64, 2, 11, 40, "K2M64", scratch=_s16(64, 2, 11, 40), ksplit=3, reduce="vec16", epi="nobias"),
    C("k2big_planned_row_cut", "k2", 44, 160, 4, 118, 252, "K2Big", scratch=_s16(160, 4, 118, 252), ksplit=3, cut=True, reduce="vec16", epi="relu+res"),
    C("k2flatbig", "k2", 12, 128, 12, 60, 108, "K2FlatBig", scratch=_s16(128, 12, 60, 108), epi="relu+res"),
    C("k2flatbig_shift", "k2", 12, 128, 12, 60, 108, "K2Big", inp="shift", scratch=_s16(128, 12, 60, 108), epi="relu+res", pair="k2flatbig", bits=True),
    C("k2flatbig56_splitk2", "k2", 12, 128, 24, 30, 52, "K2FlatBig56", scratch=_s16(128, 24, 30, 52), ksplit=2, reduce="vec16"),
    C("k2flatbig56_shift", "k2", 12, 128, 24, 30, 52, "K2Big", inp="shift", scratch=_s16(128, 24, 30, 52), ksplit=2, reduce="vec16",
      pair="k2flatbig56_splitk2", bits=True),
    C("k2flatmed", "k2", 12, 160, 2, 17, 70, "K2FlatMed", epi="nobias"),
    C("k2flatmed_shift", "k2", 12, 160, 2, 17, 70, "K2Small", inp="shift", epi="nobias", pair="k2flatmed", bits=True),
    C("k2flatmed56", "k2", 12, 128, 2, 17, 50, "K2FlatMed56", epi="relu+reshalo"),
    C("k2flatmed56_shift", "k2", 12, 128, 2, 17, 50, "K2Small", inp="shift", epi="relu+reshalo", pair="k2flatmed56", bits=True),
    C("k2flatmed56_splitk", "k2", 20, 128, 2, 17, 50, "K2FlatMed56", scratch=_s16(128, 2, 17, 50), ksplit=2, reduce="scalar", epi="relu+res"),
    C("k2_gn8_splitk", "k2", 20, 128, 2, 11, 40, "K2Small", cfg=3, scratch=_s16(128, 2, 11, 40), ksplit=2, reduce="vec16", epi="gn8"),
    # ---- 1x1x1 on the flat [C][V] view (V = T * H * W) ---------------------------------------------------------------------------------------------
    # register-staged tiles by unaligned input (V = 1001 makes every channel row misaligned), GL twins by aligned input, Cin % 16 == 0, Cout % MT == 0
    C("k1big_unaligned", "k1", 12, 160, 1, 1, 1001, "K1Big", cfg=1),
    C("k1small_unaligned", "k1", 12, 160, 1, 1, 1001, "K1Small", cfg=2, epi="relu+res"),
    C("k1small_v5", "k1", 12, 160, 1, 1, 5, "K1Small", epi="nobias"),
    C("k1m64_unaligned", "k1", 12, 64, 1, 1, 1001, "K1M64", epi="relu"),
    C("k1m64_co32_shift", "k1", 12, 32, 1, 1, 1000, "K1M64", inp="shift"),
    C("k1big_gl", "k1", 48, 128, 1, 1, 1000, "K1BigGL", cfg=1, epi="relu+res"),
    C("k1big_cin12_falls_to_staged", "k1", 12, 128, 1, 1, 1000, "K1Big", cfg=1),
    C("k1big_co160_falls_to_staged", "k1", 48, 160, 1, 1, 1000, "K1Big", cfg=1),
    C("k1big_shift_falls_to_staged", "k1", 48, 128, 1, 1, 1000, "K1Big", cfg=1, inp="shift", epi="relu+res", pair="k1big_gl", bits=True),
    C("k1small_gl", "k1", 48, 128, 1, 1, 1000, "K1SmallGL", cfg=2, epi="nobias"),
    C("k1m64_gl", "k1", 48, 64, 1, 1, 1000, "K1M64GL"),
    # the flat-decode epilogue into the interior of a zero-haloed 2-D volume, plain and through the split-K reduce
    C("k1small_decode", "k1", 12, 160, 2, 9, 37, "K1Small", epi="decode+relu+res", out="interior"),
    C("k1small_gl_decode", "k1", 48, 128, 2, 9, 38, "K1SmallGL", epi="decode+relu+reshalo", out="interior"),
    C("k1small_decode_splitk", "k1", 80, 128, 2, 9, 37, "K1Small", epi="decode+relu+res", out="interior", scratch=_s16(128, 2, 9, 37), ksplit=2,
      reduce="scalar"),
    C("k1small_gl_splitk4", "k1", 64, 128, 1, 1, 1000, "K1SmallGL", cfg=2, scratch=_s16(128, 1, 1, 1000), ksplit=4, reduce="vec16", epi="relu+res"),
    C("k1_gn4_tile", "k1", 48, 128, 1, 1, 1000, "K1SmallGL", cfg=2, epi="gn4"),
]
CASES_BY_NAME = {c.name: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)

# the short-K expansion rule of the 1x1 choice (Cin <= 256 && Cout >= 4 Cin) on both sides of its 2048-workgroup limit: plans only, no numeric case
K1_EXPANSION_RULE = [
    C("k1_expansion_below_2048", "k1", 64, 256, 1, 1, 256 * 1023, "K1SmallGL"),
    C("k1_expansion_at_2048", "k1", 64, 256, 1, 1, 256 * 1024, "K1BigGL"),
    C("k1_square_not_expansion", "k1", 64, 128, 1, 1, 256 * 600, "K1BigGL"),
]

# the f32 layer shapes at the bench sizes (printed by the host test, for the record): T = 8 at 480 x 864 -- the encoder's 3x3 convs per level, the
# decoders' 3x3x3 stages at the 4x / 8x / 16x / 32x maps -- and the KITTI 608 x 1952 4x map
PRODUCTION = [
    C("enc_layer1_3x3_4x", "k2", 64, 64, 8, 120, 216, None), C("enc_layer2_3x3_8x", "k2", 128, 128, 8, 60, 108, None),
    C("enc_layer3_3x3_16x", "k2", 256, 256, 8, 30, 54, None), C("enc_layer4_3x3_32x", "k2", 512, 512, 8, 15, 27, None),
    C("dec_block_4x", "k3", 256, 128, 8, 120, 216, None, epi="gn8"), C("dec_block_8x", "k3", 256, 128, 8, 60, 108, None, epi="gn8"),
    C("dec_block_16x", "k3", 256, 128, 8, 30, 54, None, epi="gn8"), C("dec_block_32x", "k3", 256, 128, 8, 15, 27, None, epi="gn8"),
    C("kitti_block_4x", "k3", 256, 128, 8, 152, 488, None, epi="gn8"),
]

# ---------------------------------------------------------------------------------------------------------------- the split-mode files
# Shape tuples of tests/test_gpu_bf16x6.py and tests/test_gpu_t_halo_skip.py (imported there), and -- split_file_legs() -- every conv launch
# those files make, as cases: the host census asks which split tile each one plans, and which f32 plan each yardstick leg resolves to.
X6_TILE_SHAPES = {"k1": (256, 128, 4, 30, 54), "k3": (64, 128, 3, 21, 40), "k2": (64, 128, 2, 17, 70)}       # (k1: V = 4 * 30 * 54)
X6_RAGGED = [("k3", 8, 64, 3, 5, 37), ("k3", 256, 128, 2, 9, 40), ("k3", 12, 32, 1, 2, 3), ("k3", 16, 160, 4, 17, 70),
             ("k2", 8, 64, 2, 9, 37), ("k2", 256, 256, 2, 6, 27), ("k2", 64, 64, 3, 17, 40), ("k2", 128, 128, 8, 30, 54)]
X6_UNALIGNED = (16, 64, 2, 7, 13)
X6_DECODE = [(64, 256, 2, 9, 37), (1024, 256, 2, 6, 27), (256, 1024, 3, 15, 27)]
# (Cin, Cout, T, H, W, tile_cfg): the 256-channel 1x1 tile, forced and chosen, and the 64-channel one -- tiles no other case of that file plans
X6_1X1_TILES = [(256, 256, 1, 1, 1000, 3), (512, 256, 8, 60, 72, 0), (64, 64, 1, 1, 1001, 0)]
X6_GN = [(64, 128, 2, 9, 40), (32, 256, 8, 24, 64), (256, 128, 8, 60, 108)]
X6_BLOCK4X = (256, 128, 8, 120, 216)
X6_MAGNITUDE_SHAPE = (64, 128, 2, 17, 40)
X6_DYNRANGE = {"k1": (256, 256, 3, 30, 54), "k3": (64, 128, 3, 21, 40), "k2": (64, 128, 2, 17, 70)}
X6_FLAT = [("k2", 256, 256, 8, 30, 54, "plain"), ("k2", 128, 128, 3, 60, 108, "relu+res"), ("k2", 256, 128, 2, 120, 216, "splitk"),
           ("k2", 64, 128, 5, 17, 23, "plain")]
X6_BLOCK = [("k3", 16, 128, 3, 40, 48, "plain"), ("k3", 8, 128, 2, 120, 216, "gn"), ("k3", 12, 256, 2, 37, 50, "relu+res"),
            ("k2", 32, 128, 3, 120, 216, "plain"), ("k2", 16, 256, 2, 23, 29, "relu+res"), ("k3", 8, 128, 4, 20, 24, "splitk")]
THS_TILES = [("bf16x6", 1), ("bf16x6", 2), ("bf16x6", 3), ("f16x3", 1), ("f16x3", 2), ("f16x3", 3), ("f16x3", 6), ("f16x3", 7)]
THS_SHAPE = (20, 128, 21, 60)          # (Cin, Cout, H, W); T varies
THS_T = [1, 2, 3, 4, 8]
THS_FP64_T = 3
THS_GN = dict(T=4, groups=[16, 32], tiles=[("bf16x6", 2), ("f16x3", 1), ("f16x3", 6), ("f16x3", 7)])

Leg = collections.namedtuple("Leg", "case modes f32 zero_t_halo")      # modes: split precisions that run it; f32: it also runs as the f32 yardstick


def split_file_legs():
    """(test_split_modes_encoder_with_checkpoint_like_frozen_bn_statistics runs a whole backbone per mode through the encoder entry, not single
    conv3d launches: its f32 leg is held to the fp32 CPU oracle by tests/test_gpu_parity.py and is not listed here.)"""
    both, f16 = ("bf16x6", "f16x3"), ("f16x3",)
    legs = []

    def add(name, kind, shape, cfg=0, scratch=0, modes=both, f32=True, zth=False, **kw):
        Cin, Cout, T, H, W = shape
        legs.append(Leg(C(name, kind, Cin, Cout, T, H, W, None, cfg=cfg, scratch=scratch, **kw), modes, f32, zth))

    for kind, shape in X6_TILE_SHAPES.items():                       # test_bf16x6_every_tile_shape_vs_fp64
        for cfg in ((0, 1, 2) if kind == "k1" else (0, 1, 2, 3)):
            add("tile_shape %s cfg%d" % (kind, cfg), kind, shape, cfg)
    for kind, Cin, Cout, T, H, W in X6_RAGGED:                        # test_bf16x6_ragged_shapes_and_splitk
        for scr in (0, _s16(Cout, T, H, W)):
            add("ragged %s %s%s" % (kind, (Cin, Cout, T, H, W), " split-K" if scr else ""), kind, (Cin, Cout, T, H, W), scratch=scr)
    add("unaligned rows", "k3", X6_UNALIGNED, inp="dense")            # test_bf16x6_unaligned_input_rows
    for shape in X6_DECODE:                                           # test_bf16x6_1x1_decode_residual_relu
        add("decode %s" % (shape,), "k1", shape, epi="decode+relu+res", out="interior")
    for Cin, Cout, T, H, W, cfg in X6_1X1_TILES:                      # test_bf16x6_1x1_wide_and_narrow_tiles
        add("1x1 tiles %s cfg%d" % ((Cin, Cout, T * H * W), cfg), "k1", (Cin, Cout, T, H, W), cfg)
    for shape in X6_GN:                                               # test_bf16x6_conv_with_groupnorm_statistics (32 groups)
        for scr in (0, 8 * shape[1] * shape[2] * shape[3] * shape[4]):
            add("gn %s%s" % (shape, " split-K" if scr else ""), "k3", shape, scratch=scr, f32=False, epi="gn%d" % (shape[1] // 32))
    add("block_4x", "k3", X6_BLOCK4X, scratch=4 * 128 * 8 * 120 * 216)   # test_bf16x6_block4x_shape_is_fp32_accurate_and_deterministic
    add("magnitudes", "k3", X6_MAGNITUDE_SHAPE)                       # test_split_modes_keep_fp32_level_across_operand_magnitudes
    for kind, shape in X6_DYNRANGE.items():                           # test_split_modes_keep_fp32_level_with_per_channel_dynamic_range
        add("dynamic range %s" % kind, kind, shape, epi="nobias")
    for kind, Cin, Cout, T, H, W, form in X6_FLAT:                    # test_flat_split_tiles_vs_fp64 (tile_cfg 5 and 1)
        for cfg in (5, 1):
            add("flat %s cfg%d" % ((kind, Cin, Cout, T, H, W, form), cfg), kind, (Cin, Cout, T, H, W), cfg, modes=f16, f32=False,
                scratch=8 * Cout * T * H * W if form == "splitk" else 0, epi="relu+res" if form == "relu+res" else "")
    for kind, Cin, Cout, T, H, W, form in X6_BLOCK:                   # test_block_tiles_vs_fp64 (tile_cfg 6, 1 and, 3x3x3 plain / residual, 7)
        for cfg in (6, 1) + ((7,) if kind == "k3" and form in ("plain", "relu+res") else ()):
            add("block %s cfg%d" % ((kind, Cin, Cout, T, H, W, form), cfg), kind, (Cin, Cout, T, H, W), cfg, modes=f16, f32=False,
                scratch=8 * Cout * T * H * W if form == "splitk" else 0,
                epi={"relu+res": "relu+res", "gn": "gn%d" % (Cout // 32)}.get(form, ""))
    Cin, Cout, H, W = THS_SHAPE
    for prec, cfg in THS_TILES:                                       # tests/test_gpu_t_halo_skip.py
        for T in THS_T:
            for scr in (0, _s16(Cout, T, H, W)):
                for zth in (False, True):
                    add("t-halo %s cfg%d T%d%s%s" % (prec, cfg, T, " split-K" if scr else "", " promised" if zth else ""), "k3", (Cin, Cout, T, H, W), cfg,
                        scratch=scr, modes=(prec,), f32=False, zth=zth)
    for cfg in sorted(set(c if c <= 3 else 0 for _, c in THS_TILES)):   # test_promised_vs_fp64: the f32 leg runs cfg, or 0 for the f16x3-only forms
        add("t-halo fp64 f32 leg cfg%d" % cfg, "k3", (Cin, Cout, THS_FP64_T, H, W), cfg, modes=())
    return legs


# ---------------------------------------------------------------------------------------------------------------- the split modes' own matrix
# SPLIT_CASES: the path-keyed cases of tests/test_gpu_conv_split.py, each run once per mode it lists.  A case is a Case (tile = None: the instantiation
# is per precision) and what every mode must plan for it -- Want(tile, vec4, vec_epi, ksplit, reduce) in SPLIT_PLANS, pinned by
# tests/test_conv_plan_host.py.  The list is CASES re-planned per mode (minus the planner's row cut, which is f32-only: small shapes that plan the
# same split tiles stand in), then cases until every cell of the matrix the host test prints is filled.
# epi token "stress": the activations are not N(0, 1) but magnitudes mixed over 2^-20 .. 2^17 in one tensor, both zeros, values whose f16x3
# remainder is an exact rounding tie (of the hi term and of the lo term) and values just under 2.6e5 (tests/conv_split_oracle.py).
# 3x3x3 has 4-channel chunks and the entry wants Cin % 4 == 0: no ragged last chunk exists there.  Ragged chunks: 1x3x3 Cin 12, 20, 36, 44 against
# 16 (f16x3) and 8 (bf16x6); 1x1 Cin 12, 48, 80 against 32.
# Pairs (Case.pair): the same convolution through two paths.  In the split modes EVERY pair must give equal bits:
#   * aligned / shifted twins of one tile differ in the staging only -- 16-byte pieces split by split_pair_f16 (inline assembly) against single
#     words split by split_act_f16 (plain C++), which split_operand.h claims equal bit for bit; bf16x6 uses split_bf16x3 on both;
#   * the flat and block forms keep the k order of the 16 x 32 (Y3Blk7: the 8 x 32) tile per output (conv_split_family.h), split-K aside.
Want = collections.namedtuple("Want", "tile vec4 vec_epi ksplit reduce")
SplitCase = collections.namedtuple("SplitCase", "case want")          # want: {precision: Want}
SPLIT_MODES = ("f16x3", "bf16x6")
_F16 = ("f16x3",)


def _inherited():
    drop = ("k3gl_planned", "k3gl_planned_row_cut", "k3big_planned_row_cut", "k3med_planned_row_cut", "k2big_planned_row_cut")
    for c in CASES:
        if c.name not in drop:
            yield c._replace(tile=None, bits=bool(c.pair), factor=3.0), SPLIT_MODES


def _stress_twins():
    shapes = [("y3big", "k3", 12, 128, 2, 18, 40, 1), ("y3med", "k3", 12, 128, 2, 9, 37, 2), ("y3small", "k3", 12, 32, 1, 5, 40, 3),
              ("y2big", "k2", 20, 160, 2, 18, 37, 1), ("y2med", "k2", 20, 128, 2, 9, 40, 2), ("y2small", "k2", 20, 128, 2, 5, 40, 3),
              ("y2m64", "k2", 20, 64, 2, 11, 37, 0),
              ("y1big", "k1", 48, 128, 1, 1, 1000, 1), ("y1small", "k1", 48, 160, 1, 1, 1000, 2), ("y1m64", "k1", 48, 64, 1, 1, 1000, 0),
              ("y1wide", "k1", 48, 256, 1, 1, 1000, 3)]
    for i, (n, kind, Cin, Cout, T, H, W, cfg) in enumerate(shapes):
        epi = "stress+relu" if i % 2 else "stress"
        yield C("stress_%s_aligned" % n, kind, Cin, Cout, T, H, W, None, cfg=cfg, epi=epi), SPLIT_MODES
        yield C("stress_%s_shift" % n, kind, Cin, Cout, T, H, W, None, cfg=cfg, epi=epi, inp="shift", pair="stress_%s_aligned" % n, bits=True), SPLIT_MODES


def _added():
    both, s16 = SPLIT_MODES, _s16
    A = lambda *a, modes=both, **kw: (C(*a[:7], None, **kw), modes)
    return [
        # small stand-ins for the f32 planner's row-cut shapes: wide rows (a ragged last column tile), the tiles those shapes plan in the split modes
        A("y3med_wide_rows", "k3", 12, 160, 2, 9, 250, cfg=2, epi="relu"),
        A("y2big_wide_rows", "k2", 44, 160, 2, 18, 252, cfg=1, epi="relu+res"),
        # scalar staging by a dense un-haloed input on the tiles CASES reaches it on by a shifted base only (or not at all)
        A("y3big_dense", "k3", 16, 128, 2, 18, 13, cfg=1, inp="dense", epi="relu+res"),
        A("y3med_dense", "k3", 16, 160, 2, 9, 13, cfg=2, inp="dense"),
        A("y2big_dense", "k2", 20, 128, 2, 18, 13, cfg=1, inp="dense", epi="nobias"),
        A("y2med_dense", "k2", 36, 128, 2, 9, 13, cfg=2, inp="dense", epi="relu+reshalo", out="interior"),
        A("y2m64_dense", "k2", 12, 64, 2, 11, 13, inp="dense", epi="relu"),
        A("y2med_w40_vec_epilogue", "k2", 12, 128, 2, 9, 40, cfg=2, epi="relu+res"),
        A("y2small_w40_into_interior", "k2", 12, 128, 2, 5, 40, cfg=3, out="interior"),
        # the 256-channel 1x1 tile: V = 1001 (every channel row misaligned, by-element epilogue) and V = 5
        A("y1wide_v1001", "k1", 80, 256, 1, 1, 1001, cfg=3, epi="relu+res"),
        A("y1wide_v5", "k1", 12, 256, 1, 1, 5, cfg=3, epi="nobias"),
        A("y1wide_decode", "k1", 48, 256, 2, 9, 37, cfg=3, epi="decode+relu+reshalo", out="interior"),
        A("y1big_decode_splitk", "k1", 80, 128, 2, 9, 38, cfg=1, epi="decode+relu+res", out="interior", scratch=s16(128, 2, 9, 38)),
        # GroupNorm statistics: groups of 4 and 8 channels, tile epilogue and split-K reduce, on the 1x3x3 and 1x1 tiles (3x3x3: inherited)
        A("k2_gn4_tile", "k2", 12, 128, 2, 11, 37, cfg=3, epi="gn4"),
        A("k2_gn8_tile", "k2", 12, 64, 2, 11, 40, epi="gn8"),
        A("k2_gn4_splitk", "k2", 36, 128, 2, 11, 37, cfg=3, scratch=s16(128, 2, 11, 37), epi="gn4"),
        A("k1_gn8_tile", "k1", 48, 64, 1, 1, 1001, epi="gn8"),
        A("k1_gn4_splitk", "k1", 80, 128, 1, 1, 1000, cfg=2, scratch=s16(128, 1, 1, 1000), epi="gn4"),
        A("k1_gn8_splitk", "k1", 80, 128, 1, 1, 1001, cfg=2, scratch=s16(128, 1, 1, 1001), epi="gn8"),
        # f16x3's flat form of the big 1x3x3 tile (tile_cfg 5) at the three pitch classes, each with the 16 x 32 tile on the same convolution
        A("y2flat56", "k2", 12, 128, 2, 17, 50, cfg=5, epi="relu+reshalo", out="interior", modes=_F16),
        A("y2flat56_as_2d", "k2", 12, 128, 2, 17, 50, cfg=1, epi="relu+reshalo", out="interior", pair="y2flat56", bits=True),
        A("y2flat112", "k2", 20, 128, 2, 9, 70, cfg=5, epi="nobias", modes=_F16),
        A("y2flat112_as_2d", "k2", 20, 128, 2, 9, 70, cfg=1, epi="nobias", pair="y2flat112", bits=True),
        A("y2flat224", "k2", 12, 256, 1, 5, 120, cfg=5, epi="relu+res", modes=_F16),
        A("y2flat224_as_2d", "k2", 12, 256, 1, 5, 120, cfg=1, epi="relu+res", pair="y2flat224", bits=True),
        A("y2flat56_splitk", "k2", 36, 128, 2, 17, 50, cfg=5, scratch=s16(128, 2, 17, 50), epi="relu", modes=_F16),
        # f16x3's block tiles (tile_cfg 6: 20 x 24, tile_cfg 7: 4 x 56) on ragged maps, each with the tile whose k order it keeps
        A("y3blk", "k3", 12, 128, 2, 23, 29, cfg=6, epi="relu+reshalo", out="interior", modes=_F16),
        A("y3blk_as_2d", "k3", 12, 128, 2, 23, 29, cfg=1, epi="relu+reshalo", out="interior", pair="y3blk", bits=True),
        A("y3blk_gn8", "k3", 12, 128, 2, 23, 29, cfg=6, epi="gn8", modes=_F16),
        A("y3blk_splitk", "k3", 20, 128, 1, 20, 24, cfg=6, scratch=s16(128, 1, 20, 24), epi="nobias", modes=_F16),
        A("y2blk", "k2", 20, 128, 2, 23, 29, cfg=6, epi="nobias", modes=_F16),
        A("y2blk_as_2d", "k2", 20, 128, 2, 23, 29, cfg=1, epi="nobias", pair="y2blk", bits=True),
        A("y2blk_res", "k2", 36, 256, 2, 21, 24, cfg=6, epi="relu+res", modes=_F16),
        A("y3blk7", "k3", 12, 128, 2, 9, 60, cfg=7, epi="relu+res", modes=_F16),
        A("y3blk7_as_2d", "k3", 12, 128, 2, 9, 60, cfg=2, epi="relu+res", pair="y3blk7", bits=True),
        A("y3blk7_into_interior", "k3", 12, 160, 2, 6, 57, cfg=7, epi="nobias", out="interior", modes=_F16),
    ]


SPLIT_CANDIDATES = list(_inherited()) + list(_stress_twins()) + _added()

# what every mode must plan: (tile, vec4, vec_epi, ksplit, reduce) -- written out, so that a moved threshold shows as a failing case
SPLIT_PLANS = {
    "k3big_gl_forced": {"f16x3": ("Y3Big", 1, 0, 1, None), "bf16x6": ("Y3Big", 1, 0, 1, None)},
    "k3big_gl_forced_w40": {"f16x3": ("Y3Big", 1, 1, 1, None), "bf16x6": ("Y3Big", 1, 1, 1, None)},
    "k3big_forced_shift": {"f16x3": ("Y3Big", 0, 0, 1, None), "bf16x6": ("Y3Big", 0, 0, 1, None)},
    "k3big_forced_co160": {"f16x3": ("Y3Big", 1, 0, 1, None), "bf16x6": ("Y3Big", 1, 0, 1, None)},
    "k3med_forced": {"f16x3": ("Y3Med", 1, 0, 1, None), "bf16x6": ("Y3Med", 1, 0, 1, None)},
    "k3small_forced": {"f16x3": ("Y3Small", 1, 0, 1, None), "bf16x6": ("Y3Small", 1, 0, 1, None)},
    "k3small_forced_w40": {"f16x3": ("Y3Small", 1, 1, 1, None), "bf16x6": ("Y3Small", 1, 1, 1, None)},
    "k3small_dense_unaligned": {"f16x3": ("Y3Small", 0, 0, 1, None), "bf16x6": ("Y3Small", 0, 0, 1, None)},
    "k3med_w40_vec_epilogue": {"f16x3": ("Y3Med", 1, 1, 1, None), "bf16x6": ("Y3Med", 1, 1, 1, None)},
    "k3med_w40_res_from_halo": {"f16x3": ("Y3Med", 1, 0, 1, None), "bf16x6": ("Y3Med", 1, 0, 1, None)},
    "k3med_w40_into_interior": {"f16x3": ("Y3Med", 1, 0, 1, None), "bf16x6": ("Y3Med", 1, 0, 1, None)},
    "k3flatmed": {"f16x3": ("Y3Blk7", 1, 1, 1, None), "bf16x6": ("Y3Med", 1, 1, 1, None)},
    "k3flatmed_shift": {"f16x3": ("Y3Med", 0, 1, 1, None), "bf16x6": ("Y3Med", 0, 1, 1, None)},
    "k3flatmed56": {"f16x3": ("Y3Small", 1, 0, 1, None), "bf16x6": ("Y3Small", 1, 0, 1, None)},
    "k3flatmed56_shift": {"f16x3": ("Y3Small", 0, 0, 1, None), "bf16x6": ("Y3Small", 0, 0, 1, None)},
    "k3flatsmall": {"f16x3": ("Y3Small", 1, 0, 1, None), "bf16x6": ("Y3Small", 1, 0, 1, None)},
    "k3flatsmall_shift": {"f16x3": ("Y3Small", 0, 0, 1, None), "bf16x6": ("Y3Small", 0, 0, 1, None)},
    "k3flatsmall56": {"f16x3": ("Y3Small", 1, 0, 1, None), "bf16x6": ("Y3Small", 1, 0, 1, None)},
    "k3flatsmall56_shift": {"f16x3": ("Y3Small", 0, 0, 1, None), "bf16x6": ("Y3Small", 0, 0, 1, None)},
    "k3gl_splitk16": {"f16x3": ("Y3Big", 1, 1, 16, 'vec16'), "bf16x6": ("Y3Big", 1, 1, 16, 'vec16')},
    "k3med_splitk4_by_scratch": {"f16x3": ("Y3Med", 1, 1, 4, 'vec16'), "bf16x6": ("Y3Med", 1, 1, 4, 'vec16')},
    "k3med_splitk_short_last": {"f16x3": ("Y3Med", 1, 1, 3, 'vec16'), "bf16x6": ("Y3Med", 1, 1, 3, 'vec16')},
    "k3small_splitk_scratch_off": {"f16x3": ("Y3Small", 1, 0, 3, 'scalar'), "bf16x6": ("Y3Small", 1, 0, 3, 'scalar')},
    "k3small_splitk2_w37": {"f16x3": ("Y3Small", 1, 0, 2, 'scalar'), "bf16x6": ("Y3Small", 1, 0, 2, 'scalar')},
    "k3flatsmall56_splitk": {"f16x3": ("Y3Small", 1, 0, 3, 'scalar'), "bf16x6": ("Y3Small", 1, 0, 3, 'scalar')},
    "k3flatsmall_splitk": {"f16x3": ("Y3Small", 1, 0, 3, 'scalar'), "bf16x6": ("Y3Small", 1, 0, 3, 'scalar')},
    "k3_gn4_tile": {"f16x3": ("Y3Small", 1, 0, 1, None), "bf16x6": ("Y3Small", 1, 0, 1, None)},
    "k3_gn8_tile": {"f16x3": ("Y3Med", 1, 1, 1, None), "bf16x6": ("Y3Med", 1, 1, 1, None)},
    "k3_gn4_splitk": {"f16x3": ("Y3Med", 1, 1, 3, 'vec16'), "bf16x6": ("Y3Med", 1, 1, 3, 'vec16')},
    "k3_gn8_splitk": {"f16x3": ("Y3Small", 1, 0, 3, 'scalar'), "bf16x6": ("Y3Small", 1, 0, 3, 'scalar')},
    "k2big_forced": {"f16x3": ("Y2Big", 1, 0, 1, None), "bf16x6": ("Y2Big", 1, 0, 1, None)},
    "k2med_forced": {"f16x3": ("Y2Med", 1, 0, 1, None), "bf16x6": ("Y2Med", 1, 0, 1, None)},
    "k2small_forced": {"f16x3": ("Y2Small", 1, 0, 1, None), "bf16x6": ("Y2Small", 1, 0, 1, None)},
    "k2small_dense_unaligned": {"f16x3": ("Y2Small", 0, 0, 1, None), "bf16x6": ("Y2Small", 0, 0, 1, None)},
    "k2m64": {"f16x3": ("Y2M64", 1, 0, 1, None), "bf16x6": ("Y2M64", 1, 0, 1, None)},
    "k2m64_co32_w40": {"f16x3": ("Y2M64", 1, 1, 1, None), "bf16x6": ("Y2M64", 1, 1, 1, None)},
    "k2small_splitk_w37": {"f16x3": ("Y2Small", 1, 0, 2, 'scalar'), "bf16x6": ("Y2Small", 1, 0, 2, 'scalar')},
    "k2m64_splitk_w40": {"f16x3": ("Y2M64", 1, 1, 2, 'vec16'), "bf16x6": ("Y2M64", 1, 1, 3, 'vec16')},
    "k2flatbig": {"f16x3": ("Y2Big", 1, 1, 1, None), "bf16x6": ("Y2Big", 1, 1, 1, None)},
    "k2flatbig_shift": {"f16x3": ("Y2Big", 0, 1, 1, None), "bf16x6": ("Y2Big", 0, 1, 1, None)},
    "k2flatbig56_splitk2": {"f16x3": ("Y2Flat56", 1, 0, 1, None), "bf16x6": ("Y2Big", 1, 1, 2, 'vec16')},
    "k2flatbig56_shift": {"f16x3": ("Y2Big", 0, 1, 1, None), "bf16x6": ("Y2Big", 0, 1, 2, 'vec16')},
    "k2flatmed": {"f16x3": ("Y2Small", 1, 0, 1, None), "bf16x6": ("Y2Small", 1, 0, 1, None)},
    "k2flatmed_shift": {"f16x3": ("Y2Small", 0, 0, 1, None), "bf16x6": ("Y2Small", 0, 0, 1, None)},
    "k2flatmed56": {"f16x3": ("Y2Small", 1, 0, 1, None), "bf16x6": ("Y2Small", 1, 0, 1, None)},
    "k2flatmed56_shift": {"f16x3": ("Y2Small", 0, 0, 1, None), "bf16x6": ("Y2Small", 0, 0, 1, None)},
    "k2flatmed56_splitk": {"f16x3": ("Y2Small", 1, 0, 2, 'scalar'), "bf16x6": ("Y2Small", 1, 0, 2, 'scalar')},
    "k2_gn8_splitk": {"f16x3": ("Y2Small", 1, 1, 2, 'vec16'), "bf16x6": ("Y2Small", 1, 1, 2, 'vec16')},
    "k1big_unaligned": {"f16x3": ("Y1Big", 0, 0, 1, None), "bf16x6": ("Y1Big", 0, 0, 1, None)},
    "k1small_unaligned": {"f16x3": ("Y1Small", 0, 0, 1, None), "bf16x6": ("Y1Small", 0, 0, 1, None)},
    "k1small_v5": {"f16x3": ("Y1Small", 0, 0, 1, None), "bf16x6": ("Y1Small", 0, 0, 1, None)},
    "k1m64_unaligned": {"f16x3": ("Y1M64", 0, 0, 1, None), "bf16x6": ("Y1M64", 0, 0, 1, None)},
    "k1m64_co32_shift": {"f16x3": ("Y1M64", 0, 1, 1, None), "bf16x6": ("Y1M64", 0, 1, 1, None)},
    "k1big_gl": {"f16x3": ("Y1Big", 1, 1, 1, None), "bf16x6": ("Y1Big", 1, 1, 1, None)},
    "k1big_cin12_falls_to_staged": {"f16x3": ("Y1Big", 1, 1, 1, None), "bf16x6": ("Y1Big", 1, 1, 1, None)},
    "k1big_co160_falls_to_staged": {"f16x3": ("Y1Big", 1, 1, 1, None), "bf16x6": ("Y1Big", 1, 1, 1, None)},
    "k1big_shift_falls_to_staged": {"f16x3": ("Y1Big", 0, 1, 1, None), "bf16x6": ("Y1Big", 0, 1, 1, None)},
    "k1small_gl": {"f16x3": ("Y1Small", 1, 1, 1, None), "bf16x6": ("Y1Small", 1, 1, 1, None)},
    "k1m64_gl": {"f16x3": ("Y1M64", 1, 1, 1, None), "bf16x6": ("Y1M64", 1, 1, 1, None)},
    "k1small_decode": {"f16x3": ("Y1Small", 0, 0, 1, None), "bf16x6": ("Y1Small", 0, 0, 1, None)},
    "k1small_gl_decode": {"f16x3": ("Y1Small", 1, 0, 1, None), "bf16x6": ("Y1Small", 1, 0, 1, None)},
    "k1small_decode_splitk": {"f16x3": ("Y1Small", 0, 0, 2, 'scalar'), "bf16x6": ("Y1Small", 0, 0, 2, 'scalar')},
    "k1small_gl_splitk4": {"f16x3": ("Y1Small", 1, 1, 2, 'vec16'), "bf16x6": ("Y1Small", 1, 1, 2, 'vec16')},
    "k1_gn4_tile": {"f16x3": ("Y1Small", 1, 1, 1, None), "bf16x6": ("Y1Small", 1, 1, 1, None)},
    "stress_y3big_aligned": {"f16x3": ("Y3Big", 1, 1, 1, None), "bf16x6": ("Y3Big", 1, 1, 1, None)},
    "stress_y3big_shift": {"f16x3": ("Y3Big", 0, 1, 1, None), "bf16x6": ("Y3Big", 0, 1, 1, None)},
    "stress_y3med_aligned": {"f16x3": ("Y3Med", 1, 0, 1, None), "bf16x6": ("Y3Med", 1, 0, 1, None)},
    "stress_y3med_shift": {"f16x3": ("Y3Med", 0, 0, 1, None), "bf16x6": ("Y3Med", 0, 0, 1, None)},
    "stress_y3small_aligned": {"f16x3": ("Y3Small", 1, 1, 1, None), "bf16x6": ("Y3Small", 1, 1, 1, None)},
    "stress_y3small_shift": {"f16x3": ("Y3Small", 0, 1, 1, None), "bf16x6": ("Y3Small", 0, 1, 1, None)},
    "stress_y2big_aligned": {"f16x3": ("Y2Big", 1, 0, 1, None), "bf16x6": ("Y2Big", 1, 0, 1, None)},
    "stress_y2big_shift": {"f16x3": ("Y2Big", 0, 0, 1, None), "bf16x6": ("Y2Big", 0, 0, 1, None)},
    "stress_y2med_aligned": {"f16x3": ("Y2Med", 1, 1, 1, None), "bf16x6": ("Y2Med", 1, 1, 1, None)},
    "stress_y2med_shift": {"f16x3": ("Y2Med", 0, 1, 1, None), "bf16x6": ("Y2Med", 0, 1, 1, None)},
    "stress_y2small_aligned": {"f16x3": ("Y2Small", 1, 1, 1, None), "bf16x6": ("Y2Small", 1, 1, 1, None)},
    "stress_y2small_shift": {"f16x3": ("Y2Small", 0, 1, 1, None), "bf16x6": ("Y2Small", 0, 1, 1, None)},
    "stress_y2m64_aligned": {"f16x3": ("Y2M64", 1, 0, 1, None), "bf16x6": ("Y2M64", 1, 0, 1, None)},
    "stress_y2m64_shift": {"f16x3": ("Y2M64", 0, 0, 1, None), "bf16x6": ("Y2M64", 0, 0, 1, None)},
    "stress_y1big_aligned": {"f16x3": ("Y1Big", 1, 1, 1, None), "bf16x6": ("Y1Big", 1, 1, 1, None)},
    "stress_y1big_shift": {"f16x3": ("Y1Big", 0, 1, 1, None), "bf16x6": ("Y1Big", 0, 1, 1, None)},
    "stress_y1small_aligned": {"f16x3": ("Y1Small", 1, 1, 1, None), "bf16x6": ("Y1Small", 1, 1, 1, None)},
    "stress_y1small_shift": {"f16x3": ("Y1Small", 0, 1, 1, None), "bf16x6": ("Y1Small", 0, 1, 1, None)},
    "stress_y1m64_aligned": {"f16x3": ("Y1M64", 1, 1, 1, None), "bf16x6": ("Y1M64", 1, 1, 1, None)},
    "stress_y1m64_shift": {"f16x3": ("Y1M64", 0, 1, 1, None), "bf16x6": ("Y1M64", 0, 1, 1, None)},
    "stress_y1wide_aligned": {"f16x3": ("Y1Wide", 1, 1, 1, None), "bf16x6": ("Y1Wide", 1, 1, 1, None)},
    "stress_y1wide_shift": {"f16x3": ("Y1Wide", 0, 1, 1, None), "bf16x6": ("Y1Wide", 0, 1, 1, None)},
    "y3med_wide_rows": {"f16x3": ("Y3Med", 1, 0, 1, None), "bf16x6": ("Y3Med", 1, 0, 1, None)},
    "y2big_wide_rows": {"f16x3": ("Y2Big", 1, 1, 1, None), "bf16x6": ("Y2Big", 1, 1, 1, None)},
    "y3big_dense": {"f16x3": ("Y3Big", 0, 0, 1, None), "bf16x6": ("Y3Big", 0, 0, 1, None)},
    "y3med_dense": {"f16x3": ("Y3Med", 0, 0, 1, None), "bf16x6": ("Y3Med", 0, 0, 1, None)},
    "y2big_dense": {"f16x3": ("Y2Big", 0, 0, 1, None), "bf16x6": ("Y2Big", 0, 0, 1, None)},
    "y2med_dense": {"f16x3": ("Y2Med", 0, 0, 1, None), "bf16x6": ("Y2Med", 0, 0, 1, None)},
    "y2m64_dense": {"f16x3": ("Y2M64", 0, 0, 1, None), "bf16x6": ("Y2M64", 0, 0, 1, None)},
    "y2med_w40_vec_epilogue": {"f16x3": ("Y2Med", 1, 1, 1, None), "bf16x6": ("Y2Med", 1, 1, 1, None)},
    "y2small_w40_into_interior": {"f16x3": ("Y2Small", 1, 0, 1, None), "bf16x6": ("Y2Small", 1, 0, 1, None)},
    "y1wide_v1001": {"f16x3": ("Y1Wide", 0, 0, 1, None), "bf16x6": ("Y1Wide", 0, 0, 1, None)},
    "y1wide_v5": {"f16x3": ("Y1Wide", 0, 0, 1, None), "bf16x6": ("Y1Wide", 0, 0, 1, None)},
    "y1wide_decode": {"f16x3": ("Y1Wide", 0, 0, 1, None), "bf16x6": ("Y1Wide", 0, 0, 1, None)},
    "y1big_decode_splitk": {"f16x3": ("Y1Big", 1, 1, 2, 'scalar'), "bf16x6": ("Y1Big", 1, 1, 2, 'scalar')},
    "k2_gn4_tile": {"f16x3": ("Y2Small", 1, 0, 1, None), "bf16x6": ("Y2Small", 1, 0, 1, None)},
    "k2_gn8_tile": {"f16x3": ("Y2M64", 1, 1, 1, None), "bf16x6": ("Y2M64", 1, 1, 1, None)},
    "k2_gn4_splitk": {"f16x3": ("Y2Small", 1, 0, 2, 'scalar'), "bf16x6": ("Y2Small", 1, 0, 3, 'scalar')},
    "k1_gn8_tile": {"f16x3": ("Y1M64", 0, 0, 1, None), "bf16x6": ("Y1M64", 0, 0, 1, None)},
    "k1_gn4_splitk": {"f16x3": ("Y1Small", 1, 1, 2, 'vec16'), "bf16x6": ("Y1Small", 1, 1, 2, 'vec16')},
    "k1_gn8_splitk": {"f16x3": ("Y1Small", 0, 0, 2, 'scalar'), "bf16x6": ("Y1Small", 0, 0, 2, 'scalar')},
    "y2flat56": {"f16x3": ("Y2Flat56", 1, 0, 1, None)},
    "y2flat56_as_2d": {"f16x3": ("Y2Big", 1, 0, 1, None), "bf16x6": ("Y2Big", 1, 0, 1, None)},
    "y2flat112": {"f16x3": ("Y2Flat112", 1, 0, 1, None)},
    "y2flat112_as_2d": {"f16x3": ("Y2Big", 1, 0, 1, None), "bf16x6": ("Y2Big", 1, 0, 1, None)},
    "y2flat224": {"f16x3": ("Y2Flat224", 1, 0, 1, None)},
    "y2flat224_as_2d": {"f16x3": ("Y2Big", 1, 1, 1, None), "bf16x6": ("Y2Big", 1, 1, 1, None)},
    "y2flat56_splitk": {"f16x3": ("Y2Flat56", 1, 0, 2, 'scalar')},
    "y3blk": {"f16x3": ("Y3Blk", 1, 0, 1, None)},
    "y3blk_as_2d": {"f16x3": ("Y3Big", 1, 0, 1, None), "bf16x6": ("Y3Big", 1, 0, 1, None)},
    "y3blk_gn8": {"f16x3": ("Y3Blk", 1, 0, 1, None)},
    "y3blk_splitk": {"f16x3": ("Y3Blk", 1, 1, 3, 'vec16')},
    "y2blk": {"f16x3": ("Y2Blk", 1, 0, 1, None)},
    "y2blk_as_2d": {"f16x3": ("Y2Big", 1, 0, 1, None), "bf16x6": ("Y2Big", 1, 0, 1, None)},
    "y2blk_res": {"f16x3": ("Y2Blk", 1, 1, 1, None)},
    "y3blk7": {"f16x3": ("Y3Blk7", 1, 1, 1, None)},
    "y3blk7_as_2d": {"f16x3": ("Y3Med", 1, 1, 1, None), "bf16x6": ("Y3Med", 1, 1, 1, None)},
    "y3blk7_into_interior": {"f16x3": ("Y3Blk7", 1, 0, 1, None)},
}
SPLIT_CASES = [SplitCase(c, {m: Want(*SPLIT_PLANS[c.name][m]) for m in modes}) for c, modes in SPLIT_CANDIDATES]
SPLIT_BY_NAME = {s.case.name: s for s in SPLIT_CASES}
assert len(SPLIT_BY_NAME) == len(SPLIT_CASES) == len(SPLIT_PLANS)
SPLIT_RUNS = [(s.case.name, m) for s in SPLIT_CASES for m in SPLIT_MODES if m in s.want]          # the parametrisation of the GPU file


def split_family(kind, tile):
    """The family a token is counted under in the host test's (token x family) matrix."""
    if tile.startswith("Y2Flat"):
        return "flat"
    if "Blk" in tile:
        return "block"
    return {"k3": "3x3x3", "k2": "1x3x3", "k1": "1x1"}[kind]
