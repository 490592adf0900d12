"""The exact-fp32 convolution family (conv_igemm.hip, the STEMSEG_PRECISION_F32 instantiations of conv_igemm.h) against fp64, on every
tile path.  This family is the yardstick of the split modes (tests/test_gpu_bf16x6.py, tests/test_gpu_t_halo_skip.py grant their bound
relative to ITS error), the default dgrad arithmetic of body_backward and the arithmetic of the wide heads.

Cases: tests/conv_cases.py, one per path -- 22 tile instantiations, forced and chosen, the planner's row cut, split-K 2 / 3 / 4 / 16 ways
with both reduce forms, every epilogue, aligned / unaligned / shifted inputs, dense and zero-haloed outputs.  Which path a case takes is
asserted on the CPU by tests/test_conv_plan_host.py and once more here on the real addresses.

Reference: torch's fp64 convolution of the same fp32 inputs on the CPU, bias / residual / ReLU folded in in fp64.
Yardstick: NOT torch's fp32 convolution (its summation order depends on the host) but a plain fp32 restatement in numpy
(tests/conv_f32_oracle.py): one fp32 accumulator per output, the K = Cin x taps products added one at a time in K order, then the bias -- the
worst plausible summation order -- on a fixed subset of positions, all channels.  e_seq = its max-norm error against fp64 there.

Per case, output and scratch NaN-poisoned beforehand:
  (a) on the subset  max|dev - ref64| <= FACTOR * max(e_seq, 2^-24 max|ref64|), FACTOR = 3 (the factor the split modes are granted over the
      f32 kernel); the measured ratios are in the table below -- 0.19 to 1.18, the un-split launches around 1 (their k order is close to the
      sequential one; the MFMA unit's accumulation shows no worse rounding than round-to-nearest per step) and split-K launches at
      0.2 - 0.9 -- so no case has a factor of its own;
  (b) every output   |dev - ref64| <= (K + ksplit + 4) 2^-23 S, S = fp64 conv of |x| with |w|, + |b| + |res|: one rounding of at most 2^-23
      relative per accumulation step, whatever the order -- derived, loose, and it holds outside the subset too;
  (c) every output within 2e-4 absolute (the bound of the older tests: nothing weakens);
  (d) no NaN left; the halo of a zero-haloed output volume still exactly zero; a second run gives identical bits;
  (e) pairs that differ in the path only (conv_cases.Case.pair) agree on the subset within the bound of (a), and bit for bit where the k order
      per output is the same by construction: the MFMA stream of a chunk (conv_igemm.h, `compute`) runs 4-channel group -> tap -> channel
      pair, whatever CK, rows or FLAT, so a flat tile equals its 2-D twin and a 1x1 GL tile (TAPS = 1: channel pairs ascending) its staged
      twin.  K3BigGL stages 2-channel chunks -- channel pair -> tap -- and is held to (a) against K3Big, not to equal bits.
  GroupNorm cases: the statistics against numpy on the device's own output, the output to (a) - (d).

Out of scope: the clip batch (nb > 1) and plan_frames.  The public epilogue does not carry nb, and both are held bit-identical to single
launches by tests/test_gpu_invariance.py.  ReLU's keep-NaN behaviour has its own tests (tests/test_gpu_bf16x6.py).

Measured on an MI355X (ratio = e_dev / max(e_seq, 2^-24 max|ref64|)):

  case                           instantiation ksplit  e_seq      e_dev      ratio
  k3big_gl_forced                K3BigGL            1  2.159e-06  2.077e-06  0.962
  k3big_gl_forced_w40            K3BigGL            1  2.380e-06  1.791e-06  0.753
  k3big_forced_shift             K3Big              1  2.159e-06  2.410e-06  1.116
  k3big_forced_co160             K3Big              1  2.068e-06  2.242e-06  1.084
  k3med_forced                   K3Med              1  2.065e-06  2.122e-06  1.028
  k3small_forced                 K3Small            1  6.663e-07  7.853e-07  1.179
  k3small_forced_w40             K3Small            1  8.209e-07  6.505e-07  0.792
  k3small_dense_unaligned        K3Small            1  3.493e-06  3.168e-06  0.907
  k3med_w40_vec_epilogue         K3Med              1  1.992e-06  1.671e-06  0.839
  k3med_w40_res_from_halo        K3Med              1  1.992e-06  1.671e-06  0.839
  k3med_w40_into_interior        K3Med              1  1.963e-06  1.898e-06  0.967
  k3gl_planned                   K3BigGL            1  3.871e-06  4.258e-06  1.100
  k3gl_planned_row_cut           K3BigGL            3  3.853e-06  3.418e-06  0.887
  k3big_planned_row_cut          K3Big              3  4.907e-06  3.191e-06  0.650
  k3med_planned_row_cut          K3Med              2  3.569e-06  3.153e-06  0.883
  k3flatmed                      K3FlatMed          1  3.446e-06  3.725e-06  1.081
  k3flatmed_shift                K3Med              1  3.446e-06  3.725e-06  1.081
  k3flatmed56                    K3FlatMed56        1  3.740e-06  3.740e-06  1.000
  k3flatmed56_shift              K3Med              1  3.740e-06  3.740e-06  1.000
  k3flatsmall                    K3FlatSmall        1  1.861e-06  2.183e-06  1.173
  k3flatsmall_shift              K3Small            1  1.861e-06  2.183e-06  1.173
  k3flatsmall56                  K3FlatSmall56      1  1.759e-06  1.848e-06  1.051
  k3flatsmall56_shift            K3Small            1  1.759e-06  1.848e-06  1.051
  k3gl_splitk16                  K3BigGL           16  2.570e-06  4.889e-07  0.190
  k3med_splitk4_by_scratch       K3Med              4  1.821e-06  4.998e-07  0.275
  k3med_splitk_short_last        K3Med              3  2.581e-06  1.076e-06  0.417
  k3small_splitk_scratch_off     K3Small            3  2.775e-06  1.045e-06  0.377
  k3small_splitk2_w37            K3Small            2  6.274e-07  5.601e-07  0.893
  k3flatsmall56_splitk           K3FlatSmall56      3  2.282e-06  1.420e-06  0.622
  k3flatsmall_splitk             K3FlatSmall        3  2.735e-06  1.265e-06  0.463
  k3_gn4_tile                    K3FlatSmall56      1  2.703e-06  2.226e-06  0.824
  k3_gn8_tile                    K3Med              1  1.963e-06  1.898e-06  0.967
  k3_gn4_splitk                  K3Med              3  2.219e-06  1.179e-06  0.531
  k3_gn8_splitk                  K3Small            3  2.993e-06  1.082e-06  0.361
  k2big_forced                   K2Big              1  1.890e-06  1.616e-06  0.855
  k2med_forced                   K2Med              1  1.945e-06  1.945e-06  1.000
  k2small_forced                 K2Small            1  1.720e-06  1.924e-06  1.119
  k2small_dense_unaligned        K2Small            1  1.986e-06  1.802e-06  0.907
  k2m64                          K2M64              1  1.772e-06  1.289e-06  0.727
  k2m64_co32_w40                 K2M64              1  1.519e-06  1.336e-06  0.879
  k2small_splitk_w37             K2Small            2  2.138e-06  2.058e-06  0.963
  k2m64_splitk_w40               K2M64              3  2.724e-06  1.402e-06  0.515
  k2big_planned_row_cut          K2Big              3  3.744e-06  4.174e-06  1.115
  k2flatbig                      K2FlatBig          1  2.440e-06  2.660e-06  1.090
  k2flatbig_shift                K2Big              1  2.440e-06  2.660e-06  1.090
  k2flatbig56_splitk2            K2FlatBig56        2  2.247e-06  1.770e-06  0.788
  k2flatbig56_shift              K2Big              2  2.247e-06  1.770e-06  0.788
  k2flatmed                      K2FlatMed          1  1.861e-06  2.099e-06  1.128
  k2flatmed_shift                K2Small            1  1.861e-06  2.099e-06  1.128
  k2flatmed56                    K2FlatMed56        1  1.959e-06  1.959e-06  1.000
  k2flatmed56_shift              K2Small            1  1.959e-06  1.959e-06  1.000
  k2flatmed56_splitk             K2FlatMed56        2  2.351e-06  1.997e-06  0.849
  k2_gn8_splitk                  K2Small            2  2.708e-06  2.028e-06  0.749
  k1big_unaligned                K1Big              1  8.238e-07  8.243e-07  1.001
  k1small_unaligned              K1Small            1  9.501e-07  7.916e-07  0.833
  k1small_v5                     K1Small            1  5.228e-07  4.121e-07  0.788
  k1m64_unaligned                K1M64              1  7.888e-07  6.896e-07  0.874
  k1m64_co32_shift               K1M64              1  8.292e-07  8.292e-07  1.000
  k1big_gl                       K1BigGL            1  1.104e-06  1.116e-06  1.011
  k1big_cin12_falls_to_staged    K1Big              1  1.086e-06  8.274e-07  0.762
  k1big_co160_falls_to_staged    K1Big              1  1.339e-06  1.193e-06  0.891
  k1big_shift_falls_to_staged    K1Big              1  1.104e-06  1.116e-06  1.011
  k1small_gl                     K1SmallGL          1  1.406e-06  1.183e-06  0.842
  k1m64_gl                       K1M64GL            1  1.208e-06  1.285e-06  1.064
  k1small_decode                 K1Small            1  9.582e-07  8.935e-07  0.933
  k1small_gl_decode              K1SmallGL          1  1.455e-06  1.455e-06  1.000
  k1small_decode_splitk          K1Small            2  1.515e-06  1.115e-06  0.736
  k1small_gl_splitk4             K1SmallGL          4  1.468e-06  7.394e-07  0.504
  k1_gn4_tile                    K1SmallGL          1  1.460e-06  1.460e-06  1.000
"""
import numpy as np
import pytest
import torch

from tests import conv_cases as cc
from tests import conv_f32_oracle as oracle

pytestmark = pytest.mark.gpu

FACTOR = 3.0
_RESULTS = {}


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def _t(a):
    return torch.from_numpy(np.array(a))          # (a copy: the oracle's cached arrays are read-only)


def _view(buf, g):
    return torch.as_strided(buf, (g.C, g.T, g.H, g.W), (g.cs, g.ts, g.ys, 1), g.offset)


def _launch(hip, case, bufs, pw, bias, precision="f32"):
    vin, vout = cc.volume(hip, cc.in_geom(case), bufs["in"].data_ptr()), cc.volume(hip, cc.out_geom(case), bufs["out"].data_ptr())
    scratch = bufs["scratch"][case.scratch_off:case.scratch_off + case.scratch] if case.scratch else None
    e = cc.epi_set(case)
    groups = cc.gn_groups(case)
    if groups:
        return hip.conv3d_gn(vin, pw, bias, vout, cc.TAPS[case.kind], groups, 1e-5, case.cfg, scratch, precision)
    epi = dict(precision=precision, relu=int("relu" in e))
    rg = cc.res_geom(case)
    if rg is not None:
        epi.update(residual=bufs["res"][rg.offset:], res_strides=(rg.cs, rg.ts, rg.ys))
    if "decode" in e:
        epi.update(decode=(case.H, case.W))
    hip.conv3d(vin, pw, bias, vout, cc.TAPS[case.kind], case.cfg, scratch, epi)
    return None


def make_buffers(case, d):
    """The device buffers of a case, inputs written: in / out / res / scratch (flat, with their guard words), and the bias."""
    gi, go, rg = cc.in_geom(case), cc.out_geom(case), cc.res_geom(case)
    bufs = {"in": torch.zeros(gi.total, device="cuda"), "out": torch.zeros(go.total, device="cuda")}
    _view(bufs["in"], gi).copy_(_t(d["x"]))
    if rg is not None:
        bufs["res"] = torch.zeros(rg.total, device="cuda")
        _view(bufs["res"], rg).copy_(_t(d["res"]).reshape(rg.C, rg.T, rg.H, rg.W))
    if case.scratch:
        bufs["scratch"] = torch.empty(case.scratch + 4, device="cuda")
    bufs["bias"] = None if d["b"] is None else _t(d["b"]).cuda()
    return bufs


def run_on(hip, case, d, bufs, precision="f32"):
    """Runs the case twice in `precision` on poisoned output / scratch; -> dict(out [Cout][T][H][W] float32 (1x1 without decode: [Cout][1][1][V]),
    out2, stats, recs, halo_clean)."""
    go, rg = cc.out_geom(case), cc.res_geom(case)
    pw = hip.pack_conv_weight_any(_t(d["w"]).cuda(), precision)
    bias = bufs["bias"]
    recs = cc.plan(hip, case, precision, bases=(bufs["in"].data_ptr(), bufs["out"].data_ptr(), bufs["res"].data_ptr() if rg is not None else 0,
                                                bufs["scratch"].data_ptr() if case.scratch else 0))
    outs, stats, halo_clean = [], [], True
    for _ in range(2):
        if case.out == "interior":
            bufs["out"].zero_()
        else:
            bufs["out"].fill_(float("nan"))
        _view(bufs["out"], go).fill_(float("nan"))
        if case.scratch:
            bufs["scratch"].fill_(float("nan"))
        st = _launch(hip, case, bufs, pw, bias, precision)
        torch.cuda.synchronize()
        outs.append(_view(bufs["out"], go).cpu().numpy().copy())
        stats.append(None if st is None else st.cpu().numpy())
        if case.out == "interior":
            rest = bufs["out"].clone()
            _view(rest, go).zero_()
            halo_clean = halo_clean and bool((rest == 0).all())
    return dict(out=outs[0].reshape(d["ref"].shape), out2=outs[1].reshape(d["ref"].shape), stats=stats, recs=recs, halo_clean=halo_clean)


def run_case(hip, case):
    """The f32 run of a case of conv_cases.CASES (make_buffers + run_on), kept for test_paths_agree where the case is half of a pair."""
    if case.name in _RESULTS:
        return _RESULTS[case.name]
    d = oracle.reference(case)
    r = run_on(hip, case, d, make_buffers(case, d))
    if case.pair or any(c.pair == case.name for c in cc.CASES):      # (kept for test_paths_agree only)
        _RESULTS[case.name] = r
    return r


def _seam_rows(case, recs):
    return (recs[0]["row1"] - 1, recs[0]["row1"]) if case.cut else ()


def _subset_error(case, r):
    (t, y, x), seq, e_seq = oracle.yardstick(case, _seam_rows(case, r["recs"]))
    ref = oracle.reference(case)["ref"]
    floor = 2.0 ** -24 * float(np.abs(ref).max())
    e_dev = float(np.abs(r["out"][:, t, y, x].astype(np.float64) - ref[:, t, y, x]).max())
    return e_dev, e_seq, max(e_seq, floor)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_f32_conv_vs_fp64(hip, name):
    case = cc.CASES_BY_NAME[name]
    d = oracle.reference(case)
    r = run_case(hip, case)
    recs, out, ref = r["recs"], r["out"], d["ref"]
    # the path: what tests/test_conv_plan_host.py asserts on made-up addresses holds on the real ones
    assert all(cc.tile_name(q) == case.tile for q in recs) and len(recs) == (2 if case.cut else 1)
    ksplit = max(q["ksplit"] for q in recs)
    assert ksplit == case.ksplit and [q["reduce"] for q in recs if q["ksplit"] > 1] == ([case.reduce] if case.ksplit > 1 else [])
    # (d) no stray values
    assert np.isfinite(out).all(), "%d outputs are not finite" % int((~np.isfinite(out)).sum())
    assert r["halo_clean"], "the halo of the output volume was written"
    assert np.array_equal(out.view(np.uint32), r["out2"].view(np.uint32)), "a second run gives other bits"
    # (a) against the yardstick, on the subset
    e_dev, e_seq, unit = _subset_error(case, r)
    err = np.abs(out.astype(np.float64) - ref)
    print("RATIO %-30s %-13s ksplit %2d  e_seq %.3e  e_dev %.3e  ratio %.3f   (all outputs: max|err| %.3e, max err/bound(b) %.4f)"
          % (name, case.tile, ksplit, e_seq, e_dev, e_dev / unit, err.max(), float((err / ((d["K"] + ksplit + 4) * 2.0 ** -23 * d["S"] + 1e-300)).max())))
    assert e_dev <= case.factor * unit, "(a) %.3e > %g x %.3e" % (e_dev, case.factor, unit)
    # (b) the derived cap, every output
    bound = (d["K"] + ksplit + 4) * 2.0 ** -23 * d["S"]
    assert (err <= bound).all(), "(b) %d outputs beyond (K + ksplit + 4) 2^-23 S, worst %.3g x" % (int((err > bound).sum()), float((err / (bound + 1e-300)).max()))
    # (c) the old bound
    assert err.max() <= 2e-4
    # GroupNorm statistics of the device's own output
    groups = cc.gn_groups(case)
    if groups:
        st = r["stats"][0].reshape(groups, 2)
        assert np.array_equal(r["stats"][0], r["stats"][1])
        o = out.astype(np.float64).reshape(groups, -1)
        mean, rstd = o.mean(1), 1.0 / np.sqrt(o.var(1) + 1e-5)
        assert np.abs(st[:, 0] - mean).max() <= 2e-6 * max(1.0, np.abs(mean).max())
        assert np.abs(st[:, 1] - rstd).max() <= 1e-4 * rstd.max()


@pytest.mark.parametrize("name", [c.name for c in cc.CASES if c.pair])
def test_paths_agree(hip, name):
    """(e): the same convolution through two paths."""
    case = cc.CASES_BY_NAME[name]
    other = cc.CASES_BY_NAME[case.pair]
    a, b = run_case(hip, case), run_case(hip, other)
    (t, y, x), _, _ = oracle.yardstick(case, ())
    _, _, unit = _subset_error(case, a)
    diff = float(np.abs(a["out"][:, t, y, x].astype(np.float64) - b["out"][:, t, y, x]).max())
    n_diff = int((a["out"].view(np.uint32) != b["out"].view(np.uint32)).sum())
    print("PAIR %-30s %-13s vs %-30s %-13s max|diff| %.3e (%.3f of the bound's unit), differing elements %d of %d"
          % (name, case.tile, other.name, other.tile, diff, diff / unit, n_diff, a["out"].size))
    assert diff <= FACTOR * unit
    if case.bits:
        assert n_diff == 0, "same k order per output by construction: the two paths must give the same bits"
