"""Selection of the deep 3x3x3 tile (tile_cfg hip.TILE_CFG_DEEP), on the CPU through ``hip.conv3d_plan``: at the 4x shapes of the three workloads the
request plans the deep tile -- 405 workgroups per clip at 120 x 216, 240 at 96 x 160, 1159 at 152 x 488 (the clip count of a call is the launch's
second grid dimension, StemsegDecoderDesc.n_clips, which the dry run of one convolution does not carry: its records say nb = 1) -- and the call
without the request plans what it planned before the tile existed.  tests/test_gpu_conv3d_deep_tile.py runs the tile."""
import pytest

from tests import conv_cases as cc

# (H4, W4, clips of a step, workgroups per clip of the deep tile, tile of the un-flagged call and its workgroups)
WORKLOADS = [(120, 216, 4, 405, "Y3Blk", 432), (96, 160, 4, 240, "Y3Med", 480), (152, 488, 2, 1159, "Y3Big", 1280)]


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.lib()
    return h


def _plan(hip, H, W, cfg, clips, Cin=256, Cout=128, T=8, prec="f16x3", zth=True):
    gi, go = cc.halo_geom("k3", Cin, T, H, W), cc.dense_geom(Cout, T, H, W)
    return hip.conv3d_plan(cc.volume(hip, gi, cc.BASE), cc.volume(hip, go, 2 * cc.BASE), 3, cfg, (4 * cc.BASE, 2 * Cout * T * H * W), dict(precision=prec),
                           gn_groups=32, zero_t_halo=zth, plan_clips=clips)


@pytest.mark.parametrize("H,W,clips,wgs,today,today_wgs", WORKLOADS)
def test_block4x_plans(hip, H, W, clips, wgs, today, today_wgs):
    asked = _plan(hip, H, W, hip.TILE_CFG_DEEP, clips)
    assert len(asked) == 1
    r = asked[0]
    assert (r["kt"], r["kh"], r["kw"], r["ck"], r["mt"], r["rows"], r["tw"], r["nt"], r["blk"], r["deep"], r["threads"]) == (3, 3, 3, 4, 128, 8, 8, 512, 2, 8, 512)
    assert r["grid"] == (wgs, 1, 1) and r["ksplit"] == 1 and r["gn"] == "tile epilogue" and r["zero_t_halo"] == 1 and r["vec4"] == 1 and r["vec_epi"] == 1
    plain = _plan(hip, H, W, 0, clips)
    assert len(plain) == 1 and plain[0]["deep"] == 0 and cc.tile_name(plain[0]) == today and plain[0]["grid"] == (today_wgs, 1, 1) and plain[0]["ksplit"] == 1


@pytest.mark.parametrize("kw", [dict(T=4), dict(H=60, W=108), dict(prec="bf16x6"), dict(prec="f32"), dict(zth=False), dict(H=16, W=24)],
                         ids=["T4", "60x108", "bf16x6", "f32", "no_promise", "16x24_splits_k"])
def test_request_plans_what_the_plain_call_plans(hip, kw):
    a = dict(H=120, W=216, clips=4)
    a.update(kw)
    asked, plain = _plan(hip, cfg=hip.TILE_CFG_DEEP, **a), _plan(hip, cfg=0, **a)
    assert asked == plain and all(r["deep"] == 0 for r in asked)
    for r in asked:
        cc.tile_name(r)            # (asserts that the record is one of the registered instantiations)


def test_without_the_flag_every_tile_cfg_is_unchanged(hip):
    """No tile_cfg but the request reaches the tile: the forced and automatic choices of a T = 8, 16 x 24 case name registered tiles."""
    for cfg in (0, 1, 2, 3, 6, 7):
        for r in _plan(hip, 16, 24, cfg, 1, Cin=12):
            assert r["deep"] == 0 and cc.tile_name(r) in cc.split_tiles("f16x3")
