"""The gradient-bucket kernels of csrc/optimizer.hip (pack_grads, unpack_grads, reduce_ranks) and ``GradBucket`` without a process group,
on one GPU.

Sizes 0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1 and 40000 in one table, laid out as in tests/test_gpu_optimizer.py: the CHUNK + 1 tensor is
a view one element into its storage (4-byte aligned only: two chunks on the scalar path), every gradient, destination and the bucket itself
sits in a NaN-filled buffer with guard words around it, and the bucket's own elements start as NaN too, so that a slice or a padding
element the kernel failed to write shows.  Every comparison is of bits; the expected values are computed once on the CPU."""
import logging

import numpy as np
import pytest
import torch

from tests.test_gpu_optimizer import Guarded

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 16383, 16384, 16385, 40000]
UNALIGNED = 7                   # CHUNK + 1: gradient and destination one element into their storage
MISSING = 5                     # the tensor that has no gradient in the "missing" legs (CHUNK - 1: padding behind a slice of zeros)
SPECIALS = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc01234, 0xffc00001, 0x7f800001], dtype=np.uint32).view(np.float32)
THIRD = np.float32(1.0) / np.float32(3.0)


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip
    hip.require_gpu()
    assert hip.OPT_CHUNK == 16384
    return hip


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def host_values(with_nan):
    """-0.0, the smallest and the largest denormal, both infinities (and NaNs with payloads, one of them signalling) at the head of the
    unaligned and of the largest tensor; N(0, 1) times a spread of magnitudes elsewhere."""
    rng = np.random.default_rng(7)
    vals = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 2, n)).astype(np.float32) for n in SIZES]
    sp = SPECIALS if with_nan else SPECIALS[:5]
    for i in (UNALIGNED, len(SIZES) - 1):
        vals[i][:len(sp)] = sp
    return vals


def on_device(vals, fill=None):
    """Guarded device tensors of the table's sizes: copies of ``vals``, or ``fill`` everywhere."""
    hs = [Guarded(n, shift=1 if i == UNALIGNED else 0) for i, n in enumerate(SIZES)]
    for h, v in zip(hs, vals):
        h.view.copy_(torch.from_numpy(v)) if fill is None else h.view.fill_(fill)
    return hs


def nan_bucket(total):
    b = Guarded(total)
    b.view.fill_(float("nan"))
    return b


@pytest.fixture(scope="module")
def layout(hip):
    offsets, total = hip.opt_bucket_plan(SIZES)
    assert total == sum(-(-n // 4) * 4 for n in SIZES)
    return offsets, total


def check_packed(bucket, offsets, total, expected, what):
    """expected: per tensor a float32 CPU tensor, or None for a slice of +0.0."""
    got = bits(bucket.view)
    for i, (o, n) in enumerate(zip(offsets, SIZES)):
        want = torch.zeros(n, dtype=torch.int32) if expected[i] is None else bits(expected[i])
        assert torch.equal(got[o:o + n], want), "%s: slice %d (n = %d) differs" % (what, i, n)
        end = o + -(-n // 4) * 4
        assert not got[o + n:end].any(), "%s: the padding behind slice %d is not +0.0" % (what, i)
    assert bucket.intact(), "%s: a guard word of the bucket was overwritten" % what


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.5, float(THIRD)])
def test_pack(hip, layout, scale, missing):
    offsets, total = layout
    vals = host_values(with_nan=scale == 1.0)           # (torch.equal on g * scale cannot hold a NaN; the copy is compared as bits)
    grads = on_device(vals)
    entries = [(0, 0 if (missing and i == MISSING) else h.view.data_ptr(), n) for i, (h, n) in enumerate(zip(grads, SIZES))]
    tables = hip.BucketTables(entries, "cuda")
    assert tables.total == total and tables.offsets_host == offsets
    bucket = nan_bucket(total)
    hip.opt_pack_grads(tables, bucket.view, scale)
    torch.cuda.synchronize()
    cpu = [torch.from_numpy(v) for v in vals]
    expected = [None if (missing and i == MISSING) else (g if scale == 1.0 else g * torch.tensor(np.float32(scale))) for i, g in enumerate(cpu)]
    if scale != 1.0:
        for i, (o, n) in enumerate(zip(offsets, SIZES)):
            if expected[i] is not None:
                assert torch.equal(bucket.view[o:o + n].cpu(), expected[i]), "slice %d is not g * scale in fp32" % i
    check_packed(bucket, offsets, total, expected, "scale %r" % scale)
    assert all(same_bits(h.view, g) for h, g in zip(grads, cpu)), "pack wrote into a gradient"
    assert all(h.intact() for h in grads)


def test_unpack_round_trips_the_bits_and_skips_a_null_destination(hip, layout):
    offsets, total = layout
    vals = host_values(with_nan=True)
    grads = on_device(vals)
    bucket = nan_bucket(total)
    hip.opt_pack_grads(hip.BucketTables([(0, h.view.data_ptr(), n) for h, n in zip(grads, SIZES)], "cuda"), bucket.view, 1.0)
    before = bits(bucket.view).clone()
    dests = on_device(vals, fill=123.0)
    skipped = 6                                          # CHUNK: its destination is NULL
    tables = hip.BucketTables([(0 if i == skipped else h.view.data_ptr(), 0, n) for i, (h, n) in enumerate(zip(dests, SIZES))], "cuda")
    hip.opt_unpack_grads(tables, bucket.view)
    torch.cuda.synchronize()
    for i, (h, v) in enumerate(zip(dests, vals)):
        if i == skipped:
            assert bool((h.view == 123.0).all()), "the tensor behind the NULL destination was written"
        else:
            assert same_bits(h.view, torch.from_numpy(v)), "destination %d does not hold the bits that were packed" % i
    assert all(h.intact() for h in dests) and bucket.intact() and torch.equal(bits(bucket.view), before)


def numpy_mean(rows):
    """The kernel's arithmetic restated: fp64 additions in rising rank order, one division, one rounding."""
    acc = rows[0].astype(np.float64)
    for r in rows[1:]:
        acc = acc + r.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc / np.float64(len(rows))).astype(np.float32)


@pytest.fixture(scope="module")
def rank_rows():
    """Eight ranks' values over 2 CHUNK + 9 elements, magnitudes spread over six decades so that the fp64 sum really rounds."""
    rng = np.random.default_rng(19)
    n = 2 * 16384 + 9
    return (rng.standard_normal((8, n)) * 10.0 ** rng.uniform(-4, 2, (8, n))).astype(np.float32)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_reduce_ranks_is_the_fp64_mean_in_rank_order(hip, rank_rows, world, shift):
    """shift 0 with a total that is a multiple of 4: the 16-byte path; shift 1 with an odd total: every row and the bucket 4-byte aligned
    only, the scalar path over three chunks."""
    total = 2 * 16384 + (8 if shift == 0 else 9)
    rows = rank_rows[:world, :total]
    gathered, bucket = Guarded(world * total, shift=shift), Guarded(total, shift=shift)
    gathered.view.copy_(torch.from_numpy(rows.reshape(-1)))
    bucket.view.fill_(float("nan"))
    hip.opt_reduce_ranks(gathered.view.view(world, total), bucket.view)
    torch.cuda.synchronize()
    first = bits(bucket.view).clone()
    assert torch.equal(first, bits(torch.from_numpy(numpy_mean(list(rows)))))
    bucket.view.fill_(float("nan"))
    hip.opt_reduce_ranks(gathered.view.view(world, total), bucket.view)
    torch.cuda.synchronize()
    assert torch.equal(bits(bucket.view), first), "two runs differ"
    assert gathered.intact() and bucket.intact() and same_bits(gathered.view, torch.from_numpy(rows.reshape(-1)))


@pytest.mark.parametrize("world", [1, 3])
def test_reduce_ranks_propagates_inf_and_nan(hip, rank_rows, world):
    total = 16384 + 8
    rows = rank_rows[:world, :total].copy()
    where = {5: np.inf, 16383: -np.inf, 16384: np.nan, total - 1: np.nan}           # vector body, chunk edge, the last element
    for k, (i, v) in enumerate(where.items()):
        rows[k % world, i] = v
    gathered, bucket = Guarded(world * total), Guarded(total)
    gathered.view.copy_(torch.from_numpy(rows.reshape(-1)))
    hip.opt_reduce_ranks(gathered.view.view(world, total), bucket.view)
    got = bucket.view.cpu().numpy()
    assert np.isposinf(got[5]) and np.isneginf(got[16383]) and np.isnan(got[16384]) and np.isnan(got[total - 1])
    finite = np.ones(total, bool)
    finite[list(where)] = False
    assert np.isfinite(got[finite]).all()
    keep = ~np.isnan(got)                               # (a NaN's payload is nobody's promise)
    assert np.array_equal(got.view(np.int32)[keep], numpy_mean(list(rows)).view(np.int32)[keep])


def _params(vals):
    """-> (holders, parameters) of the table's sizes, guarded."""
    holders = on_device(vals)
    params = [torch.nn.Parameter(h.view) for h in holders]
    return holders, params


def _set_grads(params, grads, holders):
    hs = on_device(grads)
    for i, (p, h) in enumerate(zip(params, hs)):
        p.grad = None if i == MISSING else h.view
    holders += hs


class _Listen(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self, logging.WARNING)
        self.said = []

    def emit(self, record):
        self.said.append(record.getMessage())


def test_grad_bucket_without_a_group_feeds_the_step_in_place(hip):
    """After ``reduce()`` every covered gradient is a view of the bucket, a DeviceSGD step from there gives the bits of a step from the
    original ``.grad``, and over three steps with fresh gradient tensors each time the optimiser uploads its tables once (momentum 0: no
    state whose first-step flag would change the key): the gradient addresses it sees do not move."""
    from stemseg_amd.training import DeviceSGD, GradBucket
    rng = np.random.default_rng(3)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    gs = [[rng.standard_normal(n).astype(np.float32) for n in SIZES] for _ in range(3)]
    ha, a = _params(p0)
    hb, b = _params(p0)
    names = ["t%d" % i for i in range(len(SIZES))]
    frozen = torch.nn.Parameter(torch.ones(5, device="cuda"), requires_grad=False)
    bucket = GradBucket(list(zip(names, a)) + [("frozen", frozen)])
    assert bucket.world == 1 and bucket.names == names and bucket.total == sum(-(-n // 4) * 4 for n in SIZES)
    opt_a, opt_b = DeviceSGD(a, lr=0.1, momentum=0.0), DeviceSGD(b, lr=0.1, momentum=0.0)
    base = bucket.bucket.data_ptr()
    listen, log = _Listen(), logging.getLogger("stemseg_amd.training")
    log.addHandler(listen)
    try:
        for step in range(3):
            _set_grads(a, gs[step], ha)
            _set_grads(b, gs[step], hb)
            bucket.reduce()
            for i, (p, o) in enumerate(zip(a, bucket.offsets)):
                assert p.grad is not None and p.grad.shape == p.shape and p.grad.is_contiguous()
                assert p.grad.numel() == 0 or p.grad.data_ptr() == base + 4 * o, "the gradient of tensor %d is no view of its slice" % i
                want = torch.zeros(SIZES[i]) if i == MISSING else torch.from_numpy(gs[step][i])
                assert same_bits(p.grad, want)
            assert frozen.grad is None
            opt_a.step()
            opt_b.step()                                 # (skips the parameter without a gradient; a zero gradient leaves its bits)
            torch.cuda.synchronize()
            assert all(same_bits(x, y) for x, y in zip(a, b)), "step %d from the bucket differs from the step from .grad" % step
            opt_a.zero_grad()
    finally:
        log.removeHandler(listen)
    assert opt_a.table_uploads == 1 and opt_b.table_uploads == 3
    said = [m for m in listen.said if "GradBucket" in m]
    assert len(said) == 1 and "t%d" % MISSING in said[0] and "t0" not in said[0], said          # once, by name
    assert all(h.intact() for h in ha + hb)


def test_grad_bucket_refuses_what_the_step_refuses(hip):
    from stemseg_amd.training import GradBucket
    with pytest.raises(NotImplementedError, match="fp32 only"):
        GradBucket([("h", torch.nn.Parameter(torch.ones(4, device="cuda", dtype=torch.float16)))])
    with pytest.raises(NotImplementedError, match="runs on the GPU"):
        GradBucket([("c", torch.nn.Parameter(torch.ones(4)))])
    with pytest.raises(ValueError, match="mode"):
        GradBucket([("p", torch.nn.Parameter(torch.ones(4, device="cuda")))], mode="tree")
    with pytest.raises(ValueError, match="no parameter"):
        GradBucket([("p", torch.nn.Parameter(torch.ones(4, device="cuda"), requires_grad=False))])
