"""The encoder's streaming kernels (csrc/encoder.hip: stem_s2d, max-pool, stride-2 copy, FPN top-down add) one by one, on every form
their launch functions pick, against the plain references of tests/encoder_stream_oracle.py.  The entry points call the launch functions
stemseg_hip_encoder_forward calls; form 0 must be the form the restated predicate names, a forced form must report itself.

- Max-pool: torch CPU max_pool2d in fp32 -- equal values (+-0 compare equal), torch's NaN mask, and both forms the same bits.
- Stride-2 copy: the bits of x[:, ::2, ::2] (NaN payloads included) and of hip.subsample2.
- Top-down add: the bits of the numpy restatement of up2_blend on inputs whose fp64 sums are exact, on every form; within 6 * 2^-24 *
  (max|coarse| + max|fine|) of fp64 bilinear interpolation; ATen's NaN mask on every form.
- Space-to-depth: the whole buffer bit for bit.
Every buffer carries a 64-float sentinel margin on both sides that must keep its bits, and so must every halo word a kernel may not write.

Measured on MI355X with one value seeded wrong at a time (no address or bound changed), the per-kernel tests of this file:
- max-pool accumulators starting at 0 instead of -inf: every case of test_maxpool_vs_torch fails (the all-negative map);
- fmaxf in place of max_keep_nan in both max-pool kernels: every case of test_maxpool_vs_torch that has the non-finite maps fails (22 of
  23: the case past the clamped grid runs the finite maps only);
- the `left` tap of the 16-byte max-pool replaced by -inf: the 16-byte cases with two or more groups a row fail test_maxpool_vs_torch
  (6; one group a row has no left neighbour) and test_maxpool_forms_agree_bit_for_bit (3 of 4);
- wy_b = 0.75 at m = 0 in both two-row forms: 26 of their 36 cases of test_upsample2x_add_bits_and_bound fail -- the ten that pass have H = 2,
  where row 0 blends the one coarse row with itself, .25 h + .75 h = h to the bit on these inputs -- and 10 of the 12 cases of
  test_upsample2x_add_nonfinite, H = 2 included (an inf or NaN of coarse row 0 at weight .75 instead of 0).
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import encoder as oenc
from tests import encoder_stream_oracle as eso
from tests import synth

pytestmark = pytest.mark.gpu

MARGIN = 64
SENT = np.float32(-1234567.0)
SENT_BITS = int(np.array(SENT).view(np.uint32))


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(name, got, ref):
    bad = _bits(got) != _bits(ref)
    if bad.any():
        i = np.flatnonzero(bad.reshape(-1))
        raise AssertionError("%s: %d of %d values differ, first at flat %d: got %r ref %r" % (name, i.size, bad.size, i[0], got.reshape(-1)[i[0]],
                                                                                            ref.reshape(-1)[i[0]]))


class Slab:
    """``n`` floats on the device, ``lead`` floats past a 256-byte boundary, between two sentinel margins."""

    def __init__(self, n, lead=0, fill=SENT):
        self.n, self.off = n, MARGIN + lead
        self.whole = torch.full((self.off + n + MARGIN,), float(SENT), dtype=torch.float32, device="cuda")
        self.data = self.whole[self.off:self.off + n]
        assert self.data.data_ptr() % 16 == (4 * lead) % 16
        if fill is not SENT:
            self.data.fill_(float(fill))

    def put(self, a):
        self.data.copy_(torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1)))
        return self

    def get(self, name):
        """The data as numpy, after checking that both margins kept their bits."""
        w = self.whole.cpu().numpy()
        m = np.concatenate([w[:self.off], w[self.off + self.n:]]).view(np.uint32)
        assert (m == SENT_BITS).all(), "%s: %d margin words overwritten" % (name, np.count_nonzero(m != SENT_BITS))
        return w[self.off:self.off + self.n].copy()


def _id(kernel, *rest):
    return "-".join([kernel] + ["x".join(map(str, r)) if isinstance(r, tuple) else str(r) for r in rest])


# ------------------------------------------------------------------------------------------------ 1. max-pool and stride-2 copy
MP_KERNELS = {1: "maxpool3x3s2_kernel", 2: "maxpool3x3s2_vec4_kernel"}
SS_KERNELS = {1: "subsample2_kernel", 2: "subsample2_vec4_kernel"}
S2_SCALAR_ONLY = [(3, 2, 2), (2, 4, 6), (2, 6, 10), (5, 2, 12)]                # W % 8 != 0
S2_BOTH = [(3, 2, 8), (2, 6, 16), (5, 10, 24), (64, 4, 32)]                    # one, two, three and four float4 groups of outputs a row
S2_MISALIGNED = (64, 4, 32)                                                    # ... with the input one float past a 16-byte boundary
S2_BIG = (40, 256, 512)                                                        # 1 310 720 outputs > 4096 x 256 threads; scalar form forced
# (shape, lead floats, form asked, form expected)
S2_CASES = [(s, 0, f, 1) for s in S2_SCALAR_ONLY for f in (0, 1)] + [(s, 0, f, f or 2) for s in S2_BOTH for f in (0, 1, 2)] + \
           [(S2_MISALIGNED, 1, f, 1) for f in (0, 1)] + [(S2_BIG, 0, 1, 1)]
S2_IDS = lambda table: [_id(table[c[3]], c[0], "lead%d" % c[1], "form%d" % c[2]) for c in S2_CASES]


def _stride2(hip, fn, x, lead, form):
    planes, H, W = x.shape
    src = Slab(x.size, lead).put(x)
    dst = Slab(planes * (H // 2) * (W // 2))
    _, used = fn(src.data.view(planes, H, W), out=dst.data.view(planes, H // 2, W // 2), form=form)
    torch.cuda.synchronize()
    _same_bits("input", src.get("input"), x.reshape(-1))
    return dst.get("output").reshape(planes, H // 2, W // 2), used


def _mp_inputs(shape):
    """-> {name: map}: all negative (an accumulator that starts at 0 shows), and +-0 among negatives (the sign of a zero maximum)."""
    neg = -np.abs(eso.rand(shape, 11 + sum(shape))) - np.float32(0.125)
    zeros = neg.copy()
    zeros.reshape(-1)[::3] = 0.0
    zeros.reshape(-1)[1::5] = -0.0
    return {"negative": neg, "zeros": zeros}


def _mp_nonfinite(H, W):
    return eso.nonfinite_planes(H, W, (0, 1, H - 1), (0, 1, 7, 8, W - 2, W - 1), 21 + H + W)


def _check_maxpool(name, got, x):
    ref = eso.maxpool_ref(x)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN at %d outputs, torch %d" % (name, np.isnan(got).sum(), np.isnan(ref).sum())
    assert np.array_equal(got, ref, equal_nan=True), "%s: %d values differ from torch" % (name, np.count_nonzero(~((got == ref) | np.isnan(ref))))


@pytest.mark.parametrize("shape,lead,form,expect", S2_CASES, ids=S2_IDS(MP_KERNELS))
def test_maxpool_vs_torch(hip, shape, lead, form, expect):
    assert form or eso.stride2_form(*shape, aligned=lead == 0) == expect
    for name, x in _mp_inputs(shape).items():
        got, used = _stride2(hip, hip.maxpool3x3s2, x, lead, form)
        assert used == expect
        _check_maxpool("%s %s" % (shape, name), got, x)
    if shape != S2_BIG:
        x = _mp_nonfinite(*shape[1:])
        got, used = _stride2(hip, hip.maxpool3x3s2, x, lead, form)
        assert used == (form or eso.stride2_form(*x.shape, aligned=lead == 0))
        ref = eso.maxpool_ref(x)
        assert np.isnan(ref).any() and np.isposinf(ref).any()
        _check_maxpool("%s non-finite" % (shape,), got, x)


@pytest.mark.parametrize("shape", S2_BOTH, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_forms_agree_bit_for_bit(hip, shape):
    """... the sign of a zero maximum and the NaN mask included (a NaN's payload is the input's on both: max_keep_nan returns an operand)."""
    inputs = dict(_mp_inputs(shape), nonfinite=_mp_nonfinite(*shape[1:]))
    for name, x in inputs.items():
        a, ua = _stride2(hip, hip.maxpool3x3s2, x, 0, 1)
        b, ub = _stride2(hip, hip.maxpool3x3s2, x, 0, 2)
        assert (ua, ub) == (1, 2)
        _same_bits("max-pool %s %s: scalar vs 16-byte form" % (shape, name), b, a)


def _ss_input(shape):
    """Random bits: NaNs with payloads, infinities, denormals and both zeros among them."""
    x = np.random.RandomState(31 + sum(shape)).randint(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert np.isnan(x).any() or x.size < 512
    return x


@pytest.mark.parametrize("shape,lead,form,expect", S2_CASES, ids=S2_IDS(SS_KERNELS))
def test_subsample_bits(hip, shape, lead, form, expect):
    assert form or eso.stride2_form(*shape, aligned=lead == 0) == expect
    x = _ss_input(shape)
    got, used = _stride2(hip, hip.encoder_subsample2, x, lead, form)
    assert used == expect
    _same_bits("subsample %s" % (shape,), got, eso.subsample_ref(x))
    other = hip.subsample2(torch.from_numpy(x).cuda()[:, None]).cpu().numpy()[:, 0]            # the training path's kernel
    _same_bits("subsample %s vs hip.subsample2" % (shape,), got, other)


@pytest.mark.parametrize("fn", ["maxpool3x3s2", "encoder_subsample2"])
def test_forced_16_byte_form_refuses_what_it_cannot_run(hip, fn):
    """W % 8 != 0, a misaligned input, odd sizes: an error before any launch, the output untouched."""
    for shape, lead, form in [((2, 4, 6), 0, 2), (S2_MISALIGNED, 1, 2), ((2, 3, 8), 0, 0), ((2, 4, 7), 0, 1), ((2, 4, 8), 0, 3)]:
        planes, H, W = shape
        src, dst = Slab(planes * H * W, lead, 1.0), Slab(planes * (H // 2) * (W // 2))
        with pytest.raises(RuntimeError):
            getattr(hip, fn)(src.data.view(planes, H, W), out=dst.data.view(planes, H // 2, W // 2), form=form)
        torch.cuda.synchronize()
        assert (_bits(dst.get("output")) == SENT_BITS).all()


# ------------------------------------------------------------------------------------------------ 2. FPN top-down add
UP_KERNELS = {1: "upsample2x_add_kernel", 2: "upsample2x_add_vec4x2_kernel", 3: "upsample2x_add_dense_vec4x2_kernel"}


class Haloed:
    """A [C][T][H + 2][pitch] buffer between sentinel margins, ``lead`` floats off its aligned position; halo and interior as given."""

    def __init__(self, hip, a, halo, lead=0, pitch=None):
        self.C, self.T, self.H, self.W = a.shape
        self.pitch = pitch or eso.padded2d(*a.shape)["pitch"]
        self.ts = (self.H + 2) * self.pitch
        self.before = np.full((self.C, self.T, self.H + 2, self.pitch), halo, np.float32)
        self.before[:, :, 1:self.H + 1, 1:self.W + 1] = a
        self.slab = Slab(self.before.size, lead).put(self.before)
        n = self.before.size
        self.view = hip.Volume(self.slab.data.data_ptr() + 4 * (self.pitch + 1), self.T * self.ts, self.ts, self.pitch, self.C, self.T, self.H, self.W,
                               n - self.pitch - 1)

    def get(self, name):
        """-> (interior, the whole buffer with the interior blanked to 0)"""
        w = self.slab.get(name).reshape(self.before.shape)
        inner = w[:, :, 1:self.H + 1, 1:self.W + 1].copy()
        w[:, :, 1:self.H + 1, 1:self.W + 1] = 0
        return inner, w


def _up2_run(hip, fine, coarse, form, dense=False, lead=0, halo=SENT, pitch=None):
    """One launch -> (the fine interior afterwards, form used).  Checks what the form may touch outside the interior: nothing (in place), or
    +0.0 in the halo columns of rows 1 .. H (dense)."""
    c = Haloed(hip, coarse, SENT)                     # a coarse halo word that gets read shows in the values
    f = Haloed(hip, np.full_like(fine, SENT) if dense else fine, halo, lead, pitch)
    d = Slab(fine.size).put(fine) if dense else None
    used = hip.upsample2x_add(f.view, c.view, d.data if dense else None, form)
    torch.cuda.synchronize()
    inner, around = f.get("fine")
    expect = f.before.copy()
    expect[:, :, 1:f.H + 1, 1:f.W + 1] = 0
    if dense:
        rows = np.zeros(expect.shape, bool)
        rows[:, :, 1:f.H + 1] = True
        rows[:, :, 1:f.H + 1, 1:f.W + 1] = False
        ok = (_bits(around) == _bits(expect)) | (rows & (_bits(around) == 0))
        assert ok.all(), "dense form: %d halo words neither kept nor +0.0 in rows 1 .. H" % np.count_nonzero(~ok)
        _same_bits("dense fine map", d.get("dense"), fine.reshape(-1))
    else:
        _same_bits("halo of fine (form %d)" % used, around, expect)
    _same_bits("coarse", c.get("coarse")[1], np.where(c.before == SENT, SENT, np.float32(0)))
    return inner, used


def _up2_forms(shape, lead=0, pitch=None):
    """[(form asked, dense?, form expected)] that can run on a fine map of ``shape``."""
    C, T, H, W = shape
    g = eso.padded2d(*shape)
    pitch = pitch or g["pitch"]
    own = eso.up2_form(C * T, H, W, (H + 2) * pitch, pitch, aligned=lead == 0)
    forms = [(0, False, own), (1, False, 1)] + ([(2, False, 2)] if own == 2 else [])
    if eso.up2_form(C * T, H, W, (H + 2) * pitch, pitch, aligned=lead == 0, dense=True):
        forms += [(0, True, 3), (3, True, 3)]
    return forms


# (shape, lead, pitch): the plan's geometry; the fine view one float off (scalar only); a pitch that is no multiple of 4 (scalar only); a pitch
# with room behind the last group (the 16-byte forms stop at 4 gq)
UP_GEOMS = [(s, 0, None) for s in eso.UP2_SHAPES] + [((2, 2, 6, 12), 1, None), ((2, 1, 12, 20), 1, None), ((2, 2, 6, 12), 0, 15), ((2, 1, 12, 20), 0, 28),
                                                    ((2, 1, 2, 4), 0, 12)]
UP_CASES = [(UP_KERNELS[e], s, lead, pitch, f, dense) for s, lead, pitch in UP_GEOMS for f, dense, e in _up2_forms(s, lead, pitch)] + \
           [(UP_KERNELS[1], eso.UP2_BIG, 0, None, 1, False)]
UP_IDS = [_id(c[0], c[1], "lead%d" % c[2], "pitch%s" % c[3], "form%d" % c[4]) for c in UP_CASES]
_up2_refs = {}


def _up2_ref(shape):
    """(fine, coarse, restated result, fp64 result, bound): computed once per shape and shared."""
    if shape not in _up2_refs:
        fine, coarse = eso.up2_inputs(shape)
        r = (fine, coarse, eso.up2_restated(fine, coarse), eso.up2_fp64(fine, coarse), eso.up2_bound(fine, coarse))
        for a in r[:4]:
            a.setflags(write=False)
        _up2_refs[shape] = r
    return _up2_refs[shape]


@pytest.mark.parametrize("kernel,shape,lead,pitch,form,dense", UP_CASES, ids=UP_IDS)
def test_upsample2x_add_bits_and_bound(hip, kernel, shape, lead, pitch, form, dense):
    fine, coarse, restated, ref64, bound = _up2_ref(shape)
    got, used = _up2_run(hip, fine, coarse, form, dense, lead, SENT, pitch)
    assert UP_KERNELS[used] == kernel
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print("[up2] %-70s max|err| vs fp64 %.3e (bound %.3e)" % (_id(kernel, shape, lead, pitch, form), err, bound))
    _same_bits("%s %s vs the restated blend" % (kernel, shape), got, restated)
    assert err <= bound
    # a zero halo (the encoder's) stays zero
    got0, _ = _up2_run(hip, fine, coarse, form, dense, lead, np.float32(0), pitch)
    _same_bits("%s %s with a zero halo" % (kernel, shape), got0, restated)


@pytest.mark.parametrize("where", ["coarse", "fine"])
@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (4, 2), (4, 4), (6, 12), (8, 10)], ids=lambda s: "x".join(map(str, s)))
def test_upsample2x_add_nonfinite(hip, hw, where):
    """inf, -inf and NaN in border rows and columns of coarse, then of fine: ATen's NaN mask and infinities on every form, and every form the
    scalar form's bits outside the NaNs.  An inf in coarse column 1 makes output column 0 NaN (weight 0 x inf): no form may blend column 0
    with itself."""
    fine, coarse = eso.up2_nonfinite_inputs(*hw, where)
    ref = eso.up2_fp64(fine, coarse)
    restated = eso.up2_restated(fine, coarse)
    assert np.isnan(ref).any()
    forms = _up2_forms(fine.shape)
    assert {e for _, _, e in forms} >= ({1, 2, 3} if hw[1] % 4 == 0 else {1, 2})
    for form, dense, expect in forms:
        got, used = _up2_run(hip, fine, coarse, form, dense)
        assert used == expect
        for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            assert np.array_equal(f(got), f(ref)), "%s form %d: %s at %d outputs, ATen %d" % (hw, used, name, f(got).sum(), f(ref).sum())
        _same_bits("%s form %d vs the restated blend (NaNs blanked)" % (hw, used), np.where(np.isnan(got), np.float32(0), got),
                   np.where(np.isnan(restated), np.float32(0), restated))
        if where == "coarse" and hw[1] >= 4:
            hit = [i for i in range(coarse.shape[0]) if np.isinf(coarse[i, 0, :, 1]).any()]
            assert hit and all(np.isnan(got[i, 0, :, 0]).any() for i in hit), "form %d: coarse column 1 does not reach output column 0" % used


def test_upsample2x_add_refuses_bad_forms_and_shapes(hip):
    fine, coarse = eso.up2_inputs((2, 1, 4, 6))

    def attempt(fine, coarse, form, dense=False, lead=0, pitch=None):
        f, c = Haloed(hip, fine, SENT, lead, pitch), Haloed(hip, coarse, SENT)
        d = Slab(fine.size).put(fine) if dense else None
        with pytest.raises(RuntimeError):
            hip.upsample2x_add(f.view, c.view, d.data if dense else None, form)
        torch.cuda.synchronize()
        _same_bits("fine after a refused call", f.slab.get("fine"), f.before.reshape(-1))
    attempt(fine, coarse, 3)                                   # the dense form without a dense map
    attempt(fine, coarse, 3, dense=True)                       # W % 4 != 0
    attempt(fine, coarse, 0, dense=True)                       # ... and no other form reads a dense map
    attempt(fine, coarse, 1, dense=True)
    attempt(fine, coarse, 2, lead=1)                           # misaligned haloed rows
    attempt(fine, coarse, 2, pitch=9)                          # pitch % 4 != 0
    attempt(fine, coarse, 4)
    attempt(fine, coarse[:, :, :, :2], 0)                      # coarse not half of fine
    attempt(fine[:, :, :3], coarse, 0)                         # odd H


# ------------------------------------------------------------------------------------------------ 3. space-to-depth
S2D_SHAPES = [(1, 2, 2), (2, 4, 6), (3, 6, 10), (1, 34, 66), (2, 512, 704)]          # the last: 1 081 344 pixel pairs > 4096 x 256 threads


@pytest.mark.parametrize("shape", S2D_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_s2d_whole_buffer(hip, shape):
    T, H, W = shape
    frames = _ss_input((T, 3, H, W))
    g = eso.s2d_geometry(T, H, W)
    src = Slab(frames.size).put(frames)
    for fill in (np.float32(0), SENT):                        # the encoder's zeroed slice; a halo the kernel must leave alone
        dst = Slab(g["floats"], 0, fill)
        v = hip.Volume(dst.data.data_ptr(), g["cs"], g["ts"], g["pitch"], 12, T, H // 2 + 3, W // 2 + 3, g["floats"])
        hip.stem_s2d(src.data.view(T, 3, H, W), v)
        torch.cuda.synchronize()
        _same_bits("s2d %s fill %r" % (shape, fill), dst.get("s2d"), eso.s2d_ref(frames, fill).reshape(-1))
    _same_bits("frames", src.get("frames"), frames.reshape(-1))


# ------------------------------------------------------------------------------------------------ 4. the smallest encoder sizes
def report(name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    i = int(np.argmax(err))
    print("[parity] %-38s max|err| %.3e at %s (got %.6g ref %.6g)  max|ref| %.3g" % (name, err.max(), np.unravel_index(i, err.shape), got.flat[i], ref.flat[i],
                                                                                   np.abs(ref).max()))
    return float(err.max())


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("hw", [(32, 32), (32, 64)], ids=lambda s: "x".join(map(str, s)))
def test_encoder_smallest_sizes_vs_oracle(hip, hw, precision):
    """32 x 32 is the smallest accepted size: level maps of 8, 4, 2 and 1, the 16x level blended from a 1 x 1 coarse map (two-row form, Hc = Wc =
    1), the 8x level on the dense form with two groups a row.  R-50, T = 2, vs the CPU oracle."""
    from stemseg_amd.modeling.backbone import ResNetFPN
    H, W = hw
    bb = ResNetFPN("R-50-FPN").eval()
    bb.precision = precision
    sd = synth.synth_state_dict([(k, v.shape) for k, v in bb.state_dict().items()], 57, prefix="backbone.")
    bb.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(bb.state_dict()[k].shape) for k, v in sd.items()})
    x = torch.from_numpy(synth.synth_frames(2, H, W, seed=57).astype(np.float32)).permute(0, 3, 1, 2) - \
        torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]
    ref = oenc.resnet_fpn(x, {"backbone." + k: v for k, v in sd.items()}, "R-50-FPN")
    assert hip.encoder_stream_forms(bb._desc(2, H, W)) == eso.encoder_stream_forms(2, H, W)
    feats = bb.cuda().run_backbone(x.cuda())
    assert bb.check_workspaces()[0] == 0
    for s in (4, 8, 16, 32):
        assert tuple(feats[s].shape) == (2, 256, H // s, W // s)
        scale = max(1.0, float(ref[s].abs().max()))
        assert report("encoder T=2 %dx%d 1/%d %s" % (H, W, s, precision), feats[s].cpu().numpy() / scale, ref[s].numpy() / scale) <= 1e-4


# ------------------------------------------------------------------------------------------------ 5. the tables reach every kernel
def test_tables_name_every_kernel():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stem-seg_amd", "csrc", "encoder.hip")).read()
    in_file = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src)) - {"stem_conv7x7_mfma_kernel"}        # (the stem: tests/test_gpu_parity.py)
    named = {MP_KERNELS[c[3]] for c in S2_CASES} | {SS_KERNELS[c[3]] for c in S2_CASES} | {c[0] for c in UP_CASES} | {"stem_s2d_kernel"}
    assert named == in_file, (sorted(named), sorted(in_file))
    # both max-pool forms see every input; the scalar kernels run past their clamped grid; every top-down form at the plan's geometry, and the
    # scalar form where the view is off or the pitch is odd
    assert {c[3] for c in S2_CASES if c[0] in S2_BOTH and c[1] == 0} == {1, 2}
    assert {(c[0], c[4]) for c in UP_CASES if c[2] == 0 and c[3] is None} >= {(k, f) for k, f in ((UP_KERNELS[1], 1), (UP_KERNELS[2], 2), (UP_KERNELS[3], 3))}
    assert all(c[0] == UP_KERNELS[1] for c in UP_CASES if c[2] == 1 or c[3] == 15)
    assert np.prod(S2_BIG) // 4 > 4096 * 256 and np.prod(eso.UP2_BIG) > 4096 * 256 and S2D_SHAPES[-1][0] * 3 * S2D_SHAPES[-1][1] * S2D_SHAPES[-1][2] // 2 > 4096 * 256
