"""Which tile, split-K factor and row cut every convolution case exercises -- asked of the launch code itself, without a GPU.

``hip.conv3d_plan`` is a dry run of ``launch_conv3d``: the same dispatch, stopped in ``launch_cfg`` before the first HIP call.  The tests
below pin the case list of tests/conv_cases.py to it:

  * every case plans the instantiation (and split-K factor, reduce form, row cut) it names, so a moved threshold in ``launch_conv3d`` that
    empties a path's coverage fails here;
  * every fp32-input instantiation of conv_igemm.hip is some case's plan, and a tile added there without a case is noticed (the `using`
    lines are counted);
  * every split-staged instantiation that ``launch_split_family`` can return is planned by some case of tests/test_gpu_bf16x6.py or
    tests/test_gpu_t_halo_skip.py;
  * every launch those two files make in f32 as their yardstick resolves to a plan (instantiation, split-K or not, vec4, vec_epi) that a
    case of tests/test_gpu_conv_f32.py holds to fp64.
  * every case of the split modes' own matrix (conv_cases.SPLIT_CASES, held to fp64 by tests/test_gpu_conv_split.py) plans, in each mode it
    lists, exactly the (instantiation, vec4, vec_epi, split-K factor, reduce form) written next to it, and the matrices that list exists for
    -- (tile x vec4), (tile x vec_epi), (token x family), GroupNorm, split-K forms, ragged extents -- have no empty cell in either mode.

A NEW TILE OR A MOVED THRESHOLD IS REGISTERED HERE: add the instantiation to conv_cases.F32_TILES (or split_tiles) and a case that plans it.
Run with ``pytest -s`` to read the census: one line per case and launch."""
import ctypes
import os
import re

import pytest

from tests import conv_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stem-seg_amd", "csrc")


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.lib()
    return h


def test_plan_symbol_exported_declared_and_bound(hip):
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    assert hasattr(raw, "stemseg_hip_conv3d_plan") and "stemseg_hip_conv3d_plan" in hip.SIGNATURES and "stemseg_hip_conv3d_plan(" in header
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11
    # the record of the binding is the record of the header, field by field
    body = header[header.index("typedef struct StemsegConvPlanRecord {"):header.index("} StemsegConvPlanRecord;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for line in re.findall(r"int32_t\s+([^;]+);", body):
        declared += [re.sub(r"\[\d+\]", "", n.strip()) for n in line.split(",")]
    assert declared == [n for n, _ in hip.ConvPlanRecord._fields_]
    assert ctypes.sizeof(hip.ConvPlanRecord) == 4 * (len(declared) + 2)          # (grid holds three)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES + cc.K1_EXPANSION_RULE])
def test_expected_plan(hip, name):
    case = dict(cc.CASES_BY_NAME, **{c.name: c for c in cc.K1_EXPANSION_RULE})[name]
    recs = cc.plan(hip, case)
    for r in recs:
        print("%-30s %s" % (name, cc.describe(r)))
        assert r["precision"] == "f32" and cc.tile_name(r) == case.tile
    assert len(recs) == (2 if case.cut else 1)
    assert max(r["ksplit"] for r in recs) == case.ksplit
    if case.ksplit > 1:
        split = [r for r in recs if r["ksplit"] > 1]
        assert len(split) == 1 and split[0]["reduce"] == case.reduce
        r = split[0]
        assert r["grid"][2] == r["ksplit"] and (r["ksplit"] - 1) * r["chunks_per_split"] < r["nchunks"] <= r["ksplit"] * r["chunks_per_split"]
    if case.cut:                                     # whole rows first, the split-K rows behind them, together the whole map
        a, b = recs
        assert a["ksplit"] == 1 and a["reduce"] is None and b["ksplit"] > 1
        assert a["row0"] == 0 and a["row1"] == b["row0"] and b["row1"] == case.H and 0 < a["row1"] < case.H and a["row1"] % a["rows"] == 0
    else:
        assert recs[0]["row0"] == 0 and recs[0]["row1"] == (1 if case.kind == "k1" else case.H)
    e = cc.epi_set(case)
    want_gn = None if not cc.gn_groups(case) else ("split-K reduce" if case.ksplit > 1 else "tile epilogue")
    assert all(r["gn"] == want_gn for r in recs)
    if case.inp != "halo":
        assert all(r["vec4"] == 0 and r["gl"] == 0 and r["flat"] == 0 for r in recs), "an unaligned input takes the register-staged 2-D tiles"
    else:
        assert all(r["vec4"] == 1 for r in recs) or (case.kind == "k1" and (case.T * case.H * case.W) % 4 != 0)
    if "reshalo" in e or case.out == "interior" or "decode" in e or case.W % 4 != 0:
        assert all(r["vec_epi"] == 0 or r["ksplit"] > 1 for r in recs)          # (a split launch writes dense partial slabs: its own vec_epi)
    if case.pair:
        other = cc.CASES_BY_NAME[case.pair]
        assert (other.kind, other.Cin, other.Cout, other.T, other.H, other.W, other.epi, other.out) == \
               (case.kind, case.Cin, case.Cout, case.T, case.H, case.W, case.epi, case.out), "a pair differs in the path only"
        assert other.tile != case.tile


def test_case_list_asks_what_the_issue_lists(hip):
    """The properties the family is held to are present in the list: split-K 2, 4 and 16 ways, a short last split, a cap by the chunk count,
    both reduce forms (the scalar one by W % 4 and by a scratch pointer one float off), the reduce under bias + residual + ReLU, under the
    decode epilogue and with GroupNorm statistics of 4- and 8-channel groups, and every epilogue on a 2-D, a flat and a 1x1 tile."""
    recs = {c.name: cc.plan(hip, c) for c in cc.CASES}
    ks = set(r["ksplit"] for rs in recs.values() for r in rs)
    assert {2, 4, 16} <= ks
    split = [(c, r) for c in cc.CASES for r in recs[c.name] if r["ksplit"] > 1]
    assert any(r["nchunks"] % r["ksplit"] != 0 for _, r in split), "a short last split"
    # fewer than 16 chunks and scratch for 16 slabs: the doubling stops at ksplit * 2 <= nchunks, i.e. at the largest power of two <= nchunks
    assert any(r["nchunks"] < 16 and c.scratch >= 16 * c.Cout * c.T * c.H * c.W and not c.cut and
               r["chunks_per_split"] == -(-r["nchunks"] // (1 << (r["nchunks"].bit_length() - 1))) for c, r in split), "ksplit capped by the chunk count"
    assert any(r["reduce"] == "scalar" and c.W % 4 != 0 for c, r in split) and any(r["reduce"] == "scalar" and c.scratch_off and c.W % 4 == 0 for c, r in split)
    assert any(r["reduce"] == "vec16" for _, r in split)
    for token in ("relu+res", "decode", "gn4", "gn8"):
        assert any(token in c.epi for c, _ in split), token
    fam = lambda c, r: "k1" if c.kind == "k1" else ("flat" if r["flat"] else "2d")
    for token in ("nobias", "relu", "res", "reshalo"):
        have = set(fam(c, r) for c in cc.CASES for r in recs[c.name] if token in cc.epi_set(c))
        assert have == {"2d", "flat", "k1"}, (token, have)
    for f in ("2d", "k1"):                                     # (flat tiles have no 16-byte epilogue)
        assert set(r["vec_epi"] for c in cc.CASES for r in recs[c.name] if fam(c, r) == f and r["ksplit"] == 1) == {0, 1}
    assert any("decode" in c.epi and r["gl"] for c in cc.CASES for r in recs[c.name])
    assert {5, 1000, 1001} <= set(c.T * c.H * c.W for c in cc.CASES if c.kind == "k1"), "voxel counts that are no multiple of the tile"


def _using_lines(path, start=None, stop=None):
    text = open(path).read()
    if start:
        text = text[text.index(start):]
        text = text[:text.index(stop)]
    return re.findall(r"^\s*(?:template\s*<[^>]*>\s*)?using\s+(\w+)\s*=\s*ConvCfg<", text, flags=re.M)


def test_f32_census(hip):
    """Every fp32-input instantiation is the plan of at least one case, and the list agrees with the source."""
    in_source = _using_lines(os.path.join(CSRC, "conv_igemm.hip"))
    assert sorted(in_source) == sorted(cc.F32_TILES), "conv_igemm.hip and conv_cases.F32_TILES disagree: register the tile and give it a case"
    assert len(set(cc.F32_TILES.values())) == len(cc.F32_TILES)
    planned = {}
    for c in cc.CASES:
        for r in cc.plan(hip, c):
            planned.setdefault(cc.tile_name(r), []).append(c.name)
    for name in sorted(cc.F32_TILES):
        print("%-14s %s" % (name, ", ".join(planned.get(name, []))))
    assert set(planned) == set(cc.F32_TILES), "no case plans %s" % sorted(set(cc.F32_TILES) - set(planned))


def test_split_mode_census(hip):
    """Every SplitTiles instantiation launch_split_family can return is planned by a case of the two split-mode test files."""
    in_source = _using_lines(os.path.join(CSRC, "conv_split_family.h"), "struct SplitTiles {", "\n};")
    for prec in ("bf16x6", "f16x3"):
        table = cc.split_tiles(prec)
        names = set(n if not n.startswith("Y2Flat") else "Y2Flat" for n in table)
        assert sorted(in_source) == sorted(names), "conv_split_family.h and conv_cases.split_tiles disagree"
        assert set(cc.SPLIT_REACHABLE[prec]) <= set(table) and "Y4Stem" not in cc.SPLIT_REACHABLE[prec]
        planned = {}
        for leg in cc.split_file_legs():
            if prec in leg.modes:
                for r in cc.plan(hip, leg.case, prec, zero_t_halo=leg.zero_t_halo):
                    assert r["precision"] == prec
                    assert r["zero_t_halo"] == int(leg.zero_t_halo)
                    planned.setdefault(cc.tile_name(r), []).append(leg.case.name)
        for name in cc.SPLIT_REACHABLE[prec]:
            print("%-7s %-10s %3d launches, e.g. %s" % (prec, name, len(planned.get(name, [])), (planned.get(name) or ["-"])[0]))
        assert set(planned) == set(cc.SPLIT_REACHABLE[prec]), (prec, sorted(set(cc.SPLIT_REACHABLE[prec]) ^ set(planned)))


def test_every_f32_yardstick_leg_is_a_checked_plan(hip):
    """The two split-mode files grant their bound relative to the fp32-MFMA kernel's own error on the same case.  Every such f32 launch plans
    an (instantiation, split-K or not, vec4, vec_epi) that a case of tests/test_gpu_conv_f32.py holds to fp64."""
    covered = {}
    for c in cc.CASES:
        for r in cc.plan(hip, c):
            covered.setdefault(cc.signature(r), c.name)
    legs = [l for l in cc.split_file_legs() if l.f32]
    assert len(legs) >= 40
    missing = []
    for leg in legs:
        for r in cc.plan(hip, leg.case):
            sig = cc.signature(r)
            print("%-50s %-40s <- %s" % (leg.case.name, sig, covered.get(sig, "NOT COVERED")))
            if sig not in covered:
                missing.append((leg.case.name, sig))
    assert not missing, missing


def test_production_plans(hip):
    """For the record: the f32 plans of the layer shapes at the bench sizes, with the split-K scratch the models give them (16 slabs)."""
    for c in cc.PRODUCTION:
        for scratch in (0, 16 * c.Cout * c.T * c.H * c.W):
            recs = cc.plan(hip, c._replace(scratch=scratch))
            assert recs
            for r in recs:
                print("%-20s scratch %-10d %s" % (c.name, scratch, cc.describe(r)))


def test_alignment_is_read_from_the_addresses(hip):
    """Pointers are used for their alignment only: the same case on made-up bases of every residue plans the GL tile exactly when the input
    base is 16-byte aligned, the 16-byte epilogue exactly when output and residual are, and the 16-byte reduce exactly when the scratch is."""
    case = cc.CASES_BY_NAME["k1small_gl_splitk4"]
    for off_in in (0, 4, 8, 12, 16):
        for off_out in (0, 4, 16):
            for off_scr in (0, 4):
                (r,) = cc.plan(hip, case, bases=(cc.BASE + off_in, 2 * cc.BASE + off_out, 3 * cc.BASE, 4 * cc.BASE + off_scr))
                assert r["vec4"] == int(off_in % 16 == 0) and r["gl"] == r["vec4"]
                assert r["reduce"] == ("vec16" if off_out % 16 == 0 and off_scr % 16 == 0 else "scalar")
    case = cc.CASES_BY_NAME["k3med_w40_vec_epilogue"]
    for off_out, off_res in ((0, 0), (4, 0), (0, 4), (16, 32)):
        (r,) = cc.plan(hip, case, bases=(cc.BASE, 2 * cc.BASE + off_out, 3 * cc.BASE + off_res, 4 * cc.BASE))
        assert r["vec_epi"] == int(off_out % 16 == 0 and off_res % 16 == 0)


def test_groupnorm_and_zero_t_halo_forms(hip):
    """The GroupNorm decision of launch_conv3d_gn is visible: groups of 4 / 8 channels take the epilogue (per tile, or the split-K reduce), any other
    group size the separate pass; the zero_t_halo form reaches the kernel parameters and changes no decision; its kt check is the entry's own."""
    base = cc.CASES_BY_NAME["k3_gn8_tile"]
    vin, vout = cc.volume(hip, cc.in_geom(base), cc.BASE), cc.volume(hip, cc.out_geom(base), 2 * cc.BASE)
    for groups, want in ((base.Cout // 8, "tile epilogue"), (base.Cout // 4, "tile epilogue"), (base.Cout // 16, "separate pass"), (1, "separate pass")):
        (r,) = hip.conv3d_plan(vin, vout, 3, 2, None, dict(precision="f32"), gn_groups=groups)
        assert r["gn"] == want and cc.tile_name(r) == "K3Med"
    (r,) = hip.conv3d_plan(vin, vout, 3, 2, (4 * cc.BASE, 16 * base.Cout * 2 * 9 * 40), dict(precision="f32"), gn_groups=base.Cout // 8)
    assert r["gn"] == "split-K reduce" and r["ksplit"] > 1
    for prec in ("f32", "bf16x6", "f16x3"):
        plain = hip.conv3d_plan(vin, vout, 3, 0, None, dict(precision=prec))
        promised = hip.conv3d_plan(vin, vout, 3, 0, None, dict(precision=prec), zero_t_halo=True)
        with_stats = hip.conv3d_plan(vin, vout, 3, 0, None, dict(precision=prec), zero_t_halo=True, gn_groups=base.Cout // 8)
        assert [dict(r, zero_t_halo=0) for r in promised] == plain and all(r["zero_t_halo"] == 1 for r in promised)
        assert [dict(r, gn=None) for r in with_stats] == promised and all(r["gn"] == "tile epilogue" for r in with_stats)
    k2 = cc.CASES_BY_NAME["k2small_forced"]
    with pytest.raises(RuntimeError, match="kt == 3"):
        cc.plan(hip, k2, zero_t_halo=True)


def test_plan_refuses_what_the_launch_refuses(hip):
    case = cc.CASES_BY_NAME["k3med_forced"]
    with pytest.raises(RuntimeError, match="Cin % 4 == 0"):
        cc.plan(hip, case._replace(Cin=6))
    with pytest.raises(RuntimeError, match="unsupported"):
        hip.conv3d_plan(cc.volume(hip, cc.in_geom(case), cc.BASE), cc.volume(hip, cc.out_geom(case), 2 * cc.BASE), (3, 1, 1))
    g = cc.in_geom(case)
    bad = hip.Volume(cc.BASE, g.cs, g.ts, g.ys, g.C, g.T + 1, g.H, g.W, g.total)
    with pytest.raises(RuntimeError, match="input extents"):
        hip.conv3d_plan(bad, cc.volume(hip, cc.out_geom(case), 2 * cc.BASE), 3)


# ---------------------------------------------------------------------------------------------------------------- the split modes' own matrix
@pytest.mark.parametrize("name,prec", cc.SPLIT_RUNS)
def test_split_expected_plan(hip, name, prec):
    """Every case of conv_cases.SPLIT_CASES plans, in each mode it lists, exactly what it names."""
    sc = cc.SPLIT_BY_NAME[name]
    case, want = sc.case, sc.want[prec]
    (r,) = cc.plan(hip, case, prec)
    print("%-30s %-6s %s" % (name, prec, cc.describe(r)))
    assert r["precision"] == prec and r["row0"] == 0 and r["row1"] == (1 if case.kind == "k1" else case.H)
    assert cc.Want(cc.tile_name(r), r["vec4"], r["vec_epi"], r["ksplit"], r["reduce"]) == want
    assert want.tile in cc.SPLIT_REACHABLE[prec] and (want.reduce is None) == (want.ksplit == 1)
    if r["ksplit"] > 1:
        assert r["grid"][2] == r["ksplit"] and (r["ksplit"] - 1) * r["chunks_per_split"] < r["nchunks"] <= r["ksplit"] * r["chunks_per_split"]
    assert r["gn"] == (None if not cc.gn_groups(case) else ("split-K reduce" if r["ksplit"] > 1 else "tile epilogue"))
    assert r["vec4"] == int(case.inp == "halo" and (case.kind != "k1" or (case.T * case.H * case.W) % 4 == 0))
    assert r["flat"] == int(want.tile.startswith("Y2Flat")) and (not r["flat"] or r["vec_epi"] == 0 or r["ksplit"] > 1)
    e = cc.epi_set(case)
    if r["ksplit"] == 1 and ("reshalo" in e or case.out == "interior" or "decode" in e or case.W % 4 != 0):
        assert r["vec_epi"] == 0
    if case.pair:
        other = cc.SPLIT_BY_NAME[case.pair].case
        assert (other.kind, other.Cin, other.Cout, other.T, other.H, other.W, other.epi, other.out) == \
               (case.kind, case.Cin, case.Cout, case.T, case.H, case.W, case.epi, case.out), "a pair differs in the path only"
        assert (other.inp, other.cfg) != (case.inp, case.cfg) and case.bits


def test_split_case_list_asks_what_the_issue_lists(hip):
    """The split-mode twin of test_case_list_asks_what_the_issue_lists, as explicit matrices per mode: (tile x vec4), (tile x vec_epi at ksplit 1),
    (token x family), GroupNorm (group size x where x family), the split-K forms and the ragged extents.  A moved threshold that empties a cell
    fails here; -s prints the census."""
    k3t, k2t, k1t = ("Y3Big", "Y3Med", "Y3Small"), ("Y2Big", "Y2Med", "Y2Small", "Y2M64"), ("Y1Big", "Y1Small", "Y1M64", "Y1Wide")
    for prec in cc.SPLIT_MODES:
        runs = [(s.case, cc.plan(hip, s.case, prec)[0]) for s in cc.SPLIT_CASES if prec in s.want]
        tile = lambda r: cc.tile_name(r)
        fam = lambda c, r: cc.split_family(c.kind, tile(r))
        # ---- staging: every register-staged tile with 16-byte pieces and word by word; the word form by a shifted base and by a dense input
        print("\n%s  tile x vec4 (cases)" % prec)
        for t in k3t + k2t + k1t:
            n = [sum(1 for c, r in runs if tile(r) == t and r["vec4"] == v) for v in (0, 1)]
            print("  %-8s vec4 0: %2d   vec4 1: %2d" % (t, n[0], n[1]))
            assert n[0] and n[1], (prec, t, n)
        for kind in ("k3", "k2"):
            for inp in ("shift", "dense"):
                assert any(c.kind == kind and c.inp == inp and r["vec4"] == 0 for c, r in runs), (prec, kind, inp)
        assert any(c.kind == "k1" and c.inp == "shift" and r["vec4"] == 0 for c, r in runs)
        assert any(c.kind == "k1" and c.inp == "halo" and c.T * c.H * c.W == 1001 and r["vec4"] == 0 for c, r in runs)
        # ---- epilogue: every 2-D and 1x1 tile un-split with the 16-byte and the by-element epilogue
        print("%s  tile x vec_epi at ksplit 1 (cases)" % prec)
        for t in k3t + k2t + k1t:
            n = [sum(1 for c, r in runs if tile(r) == t and r["ksplit"] == 1 and r["vec_epi"] == v) for v in (0, 1)]
            print("  %-8s vec_epi 0: %2d   vec_epi 1: %2d" % (t, n[0], n[1]))
            assert n[0] and n[1], (prec, t, n)
        # ---- tokens x families.  conv_igemm.hip admits "interior" on a 1x1 tile through the decode epilogue only
        fams = ("3x3x3", "1x3x3", "1x1") + (("flat", "block") if prec == "f16x3" else ())
        print("%s  token x family (cases)" % prec)
        for token in ("nobias", "relu", "res", "reshalo", "interior"):
            have = {f: sum(1 for c, r in runs if fam(c, r) == f and (c.out == "interior" if token == "interior" else token in cc.epi_set(c))) for f in fams}
            print("  %-9s %s" % (token, "  ".join("%s: %2d" % kv for kv in have.items())))
            assert all(have.values()), (prec, token, have)
        dec = [(c, r) for c, r in runs if "decode" in cc.epi_set(c)]
        assert any(r["ksplit"] == 1 for _, r in dec) and any(r["ksplit"] > 1 for _, r in dec), "decode plain and through the reduce"
        # ---- GroupNorm: groups of 4 and 8 channels, in the tile epilogue and in the reduce, per family
        print("%s  GroupNorm: token x where x family (cases)" % prec)
        for token in ("gn4", "gn8"):
            for where in ("tile epilogue", "split-K reduce"):
                have = {f: sum(1 for c, r in runs if fam(c, r) == f and token in cc.epi_set(c) and r["gn"] == where) for f in ("3x3x3", "1x3x3", "1x1")}
                print("  %s %-14s %s" % (token, where, "  ".join("%s: %2d" % kv for kv in have.items())))
                assert all(have.values()), (prec, token, where, have)
        # ---- split-K
        split = [(c, r) for c, r in runs if r["ksplit"] > 1]
        print("%s  split-K: %d cases, ksplit %s" % (prec, len(split), sorted(set(r["ksplit"] for _, r in split))))
        assert any(r["reduce"] == "vec16" for _, r in split)
        assert any(r["reduce"] == "scalar" and c.W % 4 != 0 for c, r in split), "the scalar reduce by W % 4 != 0"
        assert any(r["reduce"] == "scalar" and c.scratch_off and c.W % 4 == 0 and "decode" not in c.epi for c, r in split), "... and by a scratch pointer one float off"
        assert any(r["nchunks"] % r["ksplit"] != 0 for _, r in split), "a short last split"
        assert any(r["nchunks"] < 16 and c.scratch >= 16 * c.Cout * c.T * c.H * c.W and
                   r["chunks_per_split"] == -(-r["nchunks"] // (1 << (r["nchunks"].bit_length() - 1))) for c, r in split), "ksplit capped by the chunk count"
        assert {"3x3x3", "1x3x3", "1x1"} <= set(fam(c, r) for c, r in split)
        # ---- ragged channels and voxel counts (3x3x3: 4-channel chunks and Cin % 4 == 0 at the entry -- no ragged chunk exists)
        ck2 = cc.split_tiles(prec)["Y2Big"].ck
        assert {12, 20, 36} <= set(c.Cin for c, _ in runs if c.kind == "k2") and all(n % ck2 for n in (12, 20, 36))
        assert {12, 48, 80} <= set(c.Cin for c, _ in runs if c.kind == "k1")
        assert {32, 160} <= set(c.Cout for c, _ in runs)
        assert {5, 1000, 1001} <= set(c.T * c.H * c.W for c, _ in runs if c.kind == "k1")
        assert set(tile(r) for _, r in runs) == set(cc.SPLIT_REACHABLE[prec])


def test_split_cases_keep_the_f32_list_and_their_f32_legs_are_checked_plans(hip):
    """SPLIT_CASES starts from CASES (the planner's row cut aside): the f32 leg each of those runs as the yardstick of rule (a) is a plan that
    tests/test_gpu_conv_f32.py holds to fp64.  (The cases added for the split modes run f32 plans of their own -- another tile, or a signature no
    f32 case has; tests/test_gpu_conv_split.py holds THEIR f32 leg to the f32 file's bounds (a) and (b) itself.)"""
    kept = set(cc.SPLIT_BY_NAME) & set(cc.CASES_BY_NAME)
    assert set(cc.CASES_BY_NAME) - kept == {"k3gl_planned", "k3gl_planned_row_cut", "k3big_planned_row_cut", "k3med_planned_row_cut", "k2big_planned_row_cut"}
    for name in kept:
        a, b = cc.SPLIT_BY_NAME[name].case, cc.CASES_BY_NAME[name]
        assert a._replace(tile=b.tile, bits=b.bits, factor=b.factor) == b, "the f32 leg of an inherited case is the f32 case"
        assert a.bits == bool(a.pair)
