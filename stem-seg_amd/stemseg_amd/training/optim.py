"""``DeviceSGD`` / ``DeviceAdam``: ``torch.optim.SGD`` / ``torch.optim.Adam`` whose ``step()`` is one launch per parameter group
(csrc/optimizer.hip), and ``grad_norm``: the global gradient norm and the clip coefficient of ``torch.nn.utils.clip_grad_norm_`` on the
device, without a read-back.

Constructors, ``param_groups``, ``state`` and the state dicts are the parents': the state of a ``DeviceSGD`` loads into a
``torch.optim.SGD`` and back (``momentum_buffer``), that of a ``DeviceAdam`` into ``torch.optim.Adam`` (``step`` a CPU scalar tensor,
``exp_avg``, ``exp_avg_sq``).  The arithmetic is ``_single_tensor_sgd`` / ``_single_tensor_adam`` in fp32, rounded where torch's CPU kernels
round.  What the kernels do not do is refused by name, never run through a stock path.

``GradBucket``: the gradients of data-parallel training in one flat buffer, averaged over the ranks of a process group with one
collective, and handed back as ``p.grad`` views of that buffer, which the classes above then read in place.
"""
import logging

import numpy as np
import torch
import torch.distributed as dist

from .. import hip

_TABLE_CACHE = {}               # grad_norm's tables, by key; a handful of parameter sets at most
_TABLE_CACHE_MAX = 4


def _refuse(who, what):
    raise NotImplementedError("%s: %s is not implemented by the device step (csrc/optimizer.hip); use the stock torch.optim class for it "
                              "(training.utils.create_optimizer(..., device_step=False))" % (who, what))


def _check_group_options(who, group):
    for key in ("maximize", "amsgrad", "foreach", "fused", "capturable", "differentiable", "decoupled_weight_decay"):
        if group.get(key):
            _refuse(who, "%s=%r" % (key, group[key]))


def _check_tensors(who, p, need_device=True):
    g = p.grad                      # (None only for the gradient bucket, which fills in zeros for it)
    if g is not None and g.is_sparse:
        _refuse(who, "a sparse gradient (parameter of shape %s)" % (tuple(p.shape),))
    if p.dtype != torch.float32 or (g is not None and g.dtype != torch.float32):
        _refuse(who, "a %s parameter with a %s gradient (shape %s; fp32 only)" % (p.dtype, p.dtype if g is None else g.dtype, tuple(p.shape)))
    if not p.is_contiguous():
        _refuse(who, "a non-contiguous parameter (shape %s, strides %s)" % (tuple(p.shape), tuple(p.stride())))
    if need_device and not p.is_cuda:
        _refuse(who, "a parameter on %s (shape %s): the step runs on the GPU" % (p.device, tuple(p.shape)))
    if g is not None and g.device != p.device:
        _refuse(who, "a gradient on %s for a parameter on %s" % (g.device, p.device))


def _contiguous_grads(params):
    """The gradients as the kernels read them: ``p.grad`` itself, or a contiguous copy of a strided one (kept alive by the caller)."""
    return [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params]


class _DeviceStep(object):
    """What the two classes share: per parameter group the cached tables and the launch."""

    def _tables(self, index, params, grads, states, flags, n_states):
        key = tuple((p.data_ptr(), g.data_ptr()) + tuple(s.data_ptr() for s in st) + (p.numel(), f)
                    for p, g, st, f in zip(params, grads, states, flags))
        cache = self.__dict__.setdefault("_table_cache", {})
        hit = cache.get(index)
        if hit is None or hit[0] != key:
            entries = [(p.data_ptr(), g.data_ptr()) + tuple(s.data_ptr() for s in st) + (0,) * (2 - len(st)) + (p.numel(), f)
                       for p, g, st, f in zip(params, grads, states, flags)]
            hit = cache[index] = (key, hip.OptTables(entries, n_states, params[0].device))
            self.table_uploads = getattr(self, "table_uploads", 0) + 1
        return hit[1]

    def _group_params(self, who, group):
        _check_group_options(who, group)
        params = [p for p in group["params"] if p.grad is not None]
        for p in params:
            _check_tensors(who, p)
        if len({p.device for p in params}) > 1:
            _refuse(who, "a parameter group spread over several devices")
        return params

    @staticmethod
    def _scale(grad_scale, device):
        if grad_scale is None or torch.is_tensor(grad_scale):
            if grad_scale is not None and (grad_scale.dtype != torch.float32 or grad_scale.numel() != 1 or grad_scale.device != device):
                raise ValueError("grad_scale: a float32 tensor of one element on %s, or a float" % (device,))
            return grad_scale
        return torch.full((1,), float(grad_scale), dtype=torch.float32, device=device)


class DeviceSGD(_DeviceStep, torch.optim.SGD):
    """``torch.optim.SGD`` (momentum, dampening, Nesterov, L2 weight decay) with the step on the device."""

    def __init__(self, params, *args, **kwargs):
        torch.optim.SGD.__init__(self, params, *args, **kwargs)
        for group in self.param_groups:
            _check_group_options("DeviceSGD", group)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """One launch per parameter group, no synchronisation.  grad_scale: a device float32 [1] (``grad_norm``'s coef) or a float; every
        gradient element is multiplied by it on the way in, ``.grad`` itself stays as it is."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for index, group in enumerate(self.param_groups):
            params = self._group_params("DeviceSGD", group)
            if not params:
                continue
            grads = _contiguous_grads(params)
            states, flags = [], []
            for p in params:
                if group["momentum"] != 0:
                    state = self.state[p]
                    buf = state.get("momentum_buffer")
                    fresh = buf is None
                    if fresh:
                        buf = torch.empty_like(p, memory_format=torch.contiguous_format)    # (written whole by the launch; joins the state after it)
                    elif buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != p.device:
                        _refuse("DeviceSGD", "a momentum buffer that is not a contiguous fp32 tensor on the parameter's device")
                    states.append((buf,))
                    flags.append(hip.OPT_STATE_UNINIT if fresh else 0)
                else:
                    states.append(())
                    flags.append(0)
            n_states = 1 if group["momentum"] != 0 else 0
            tables = self._tables(index, params, grads, states, flags, n_states)
            hyper = hip.opt_hyper(lr=float(group["lr"]), momentum=group["momentum"], dampening=group["dampening"],
                                  weight_decay=float(group["weight_decay"]), nesterov=group["nesterov"])
            hip.opt_sgd_step(tables, hyper, self._scale(grad_scale, params[0].device))
            # the launch is enqueued: only now do the fresh buffers count as initialised (a call that raised leaves the state as it was)
            for p, st, f in zip(params, states, flags):
                if f:
                    self.state[p]["momentum_buffer"] = st[0]
            # the kernel wrote through raw pointers: move the version counters, which the packed-operand caches are keyed on
            torch.autograd.graph.increment_version(params)
        return loss


class DeviceAdam(_DeviceStep, torch.optim.Adam):
    """``torch.optim.Adam`` (L2 weight decay, no amsgrad) with the step on the device."""

    def __init__(self, params, *args, **kwargs):
        torch.optim.Adam.__init__(self, params, *args, **kwargs)
        for group in self.param_groups:
            _check_group_options("DeviceAdam", group)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """As ``DeviceSGD.step``.  The bias corrections come from each tensor's own ``state['step']`` in Python floats, as in torch."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for index, group in enumerate(self.param_groups):
            params = self._group_params("DeviceAdam", group)
            if not params:
                continue
            grads = _contiguous_grads(params)
            beta1, beta2 = (float(b) for b in group["betas"])
            lr = float(group["lr"])
            states, scalars = [], []
            for p in params:
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                for name in ("exp_avg", "exp_avg_sq"):
                    s = state[name]
                    if s.dtype != torch.float32 or not s.is_contiguous() or s.device != p.device:
                        _refuse("DeviceAdam", "a state tensor %s that is not a contiguous fp32 tensor on the parameter's device" % name)
                step = float(state["step"]) + 1.0                        # (counted in the state once the launch is enqueued)
                scalars += [lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5]
                states.append((state["exp_avg"], state["exp_avg_sq"]))
            tables = self._tables(index, params, grads, states, [0] * len(params), 2)
            dev = params[0].device
            side = torch.tensor(scalars, dtype=torch.float32).reshape(-1, 2).pin_memory().to(dev, non_blocking=True)
            hyper = hip.opt_hyper(weight_decay=float(group["weight_decay"]), beta1=beta1, beta2=beta2, eps=group["eps"])
            hip.opt_adam_step(tables, hyper, side, self._scale(grad_scale, dev))
            for p in params:
                self.state[p]["step"] += 1
            torch.autograd.graph.increment_version(params)
        return loss


def grad_norm(parameters, max_norm=None):
    """-> (norm float64 [1], coef float32 [1], nonfinite int32 [1]) on the device: the L2 norm over the gradients of ``parameters`` (those
    whose ``.grad`` is None do not count), ``min(1, max_norm / (norm + 1e-6))`` -- ``clip_grad_norm_``'s coefficient; 1 without a
    ``max_norm`` -- and 1 when a gradient element is inf or NaN.  Nothing is read back and no gradient is touched: hand ``coef`` to
    ``DeviceSGD.step(grad_scale=coef)`` / ``DeviceAdam.step``."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        raise ValueError("grad_norm: no parameter has a gradient")
    for p in params:
        _check_tensors("grad_norm", p)
    if len({p.device for p in params}) > 1:
        _refuse("grad_norm", "parameters spread over several devices")
    grads = _contiguous_grads(params)
    key = (params[0].device,) + tuple((g.data_ptr(), g.numel()) for g in grads)
    tables = _TABLE_CACHE.get(key)
    if tables is None:
        if len(_TABLE_CACHE) >= _TABLE_CACHE_MAX:
            _TABLE_CACHE.pop(next(iter(_TABLE_CACHE)))
        tables = _TABLE_CACHE[key] = hip.OptTables([(g.data_ptr(), g.data_ptr(), 0, 0, g.numel(), 0) for g in grads], 0, params[0].device)     # (p := g: the norm reads g and n only, and the key covers both)
    return hip.opt_grad_norm(tables, max_norm)


class GradBucket(object):
    """One flat fp32 buffer for the gradients of every parameter with ``requires_grad``, in ``named_parameters`` order (the layout rule of
    include/stemseg_hip.h: a function of the sizes alone, so the same on every rank), and the average over the ranks of ``process_group``.

    ``reduce()``:
      * ``mode="allreduce"``: one launch packs ``g * float32(1 / world)`` into the buffer, one ``dist.all_reduce(SUM)`` adds the ranks.
        The products are exact to one rounding each; the order of the additions is the backend's.
      * ``mode="ordered"``: one launch packs the bits of ``g``, one all-gather collects ``[world][total]`` (the tensor form under nccl, the
        list form under any other backend), one launch adds the ranks in fp64 in rank order, divides and rounds once: the result does not
        depend on the backend.
      * world 1 or no group (``process_group=None`` with no default group initialised): the pack at scale 1 alone, plus, on a group of one
        rank, the collective.
    Afterwards ``p.grad`` of every covered parameter is a view of its slice of ``self.bucket``: ``DeviceSGD``, ``DeviceAdam``, ``grad_norm``
    and the stock optimisers read the average with no unpack pass, and the device classes' tables see the same gradient addresses at every
    step.  The bucket's own pack tables are keyed on the addresses of the local gradients: while those stay (gradients accumulated in
    place) a ``reduce()`` is the launch and the collective; when they move -- after ``zero_grad()`` and a backward pass they did, in every
    step measured -- it first rebuilds the descriptors on the host and uploads three small tables (``table_uploads`` counts these; about
    0.4 ms for 207 tensors).  A parameter without a local gradient contributes zeros and holds the average afterwards, as under DistributedDataParallel when
    a parameter goes unused on one rank; at the first ``reduce()`` the names of such parameters are logged once.  Nothing is read back.

    ``named_parameters`` may include frozen parameters: ``broadcast_parameters`` covers all of them."""

    MODES = ("allreduce", "ordered")

    def __init__(self, named_parameters, process_group=None, mode="allreduce"):
        if mode not in self.MODES:
            raise ValueError("GradBucket: mode %r is not one of %s" % (mode, self.MODES))
        self.mode, self.group = mode, process_group
        self.all_named = [(k, p) for k, p in named_parameters]
        named = [(k, p) for k, p in self.all_named if p.requires_grad]
        if not named:
            raise ValueError("GradBucket: no parameter requires a gradient")
        self.names, self.params = [k for k, _ in named], [p for _, p in named]
        for p in self.params:
            _check_tensors("GradBucket", p)
        if len({p.device for p in self.params}) > 1:
            _refuse("GradBucket", "parameters spread over several devices")
        self.device = self.params[0].device
        self.has_group = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(process_group) if self.has_group else 1
        if self.world > hip.OPT_MAX_WORLD:
            _refuse("GradBucket", "a group of %d ranks (at most %d)" % (self.world, hip.OPT_MAX_WORLD))
        self.backend = dist.get_backend(process_group) if self.has_group else None
        self.offsets, self.total = hip.opt_bucket_plan([p.numel() for p in self.params])
        self.bucket = torch.zeros(max(self.total, 4), dtype=torch.float32, device=self.device)[:self.total]
        self.views = [self.bucket[o:o + p.numel()].view_as(p) for o, p in zip(self.offsets, self.params)]
        self.gathered = None                # [world][total], the ordered mode's landing buffer
        self.table_uploads = 0
        self._tables = None                 # (key, hip.BucketTables) of the last pack
        self._said_missing = False

    def _pack_tables(self, grads):
        key = tuple(0 if g is None else g.data_ptr() for g in grads)
        if self._tables is None or self._tables[0] != key:
            self._tables = (key, hip.BucketTables([(0, a, p.numel()) for a, p in zip(key, self.params)], self.device))
            self.table_uploads += 1
        return self._tables[1]

    @torch.no_grad()
    def reduce(self):
        """Pack, reduce over the group, repoint ``p.grad``.  Enqueued on the current stream; no synchronisation of its own."""
        for p in self.params:
            _check_tensors("GradBucket", p)
        missing = [k for k, p in zip(self.names, self.params) if p.grad is None]
        if missing and not self._said_missing:
            self._said_missing = True
            logging.getLogger("stemseg_amd.training").warning(
                "GradBucket: %d of %d parameters have no gradient on this rank at the first reduce and contribute zeros: %s"
                % (len(missing), len(self.params), ", ".join(missing)))
        grads = [None if p.grad is None else (p.grad if p.grad.is_contiguous() else p.grad.contiguous()) for p in self.params]
        ordered = self.mode == "ordered"
        scale = 1.0 if ordered or self.world == 1 else float(np.float32(1.0) / np.float32(self.world))
        if self.total:
            hip.opt_pack_grads(self._pack_tables(grads), self.bucket, scale)
            if self.has_group and not ordered:
                dist.all_reduce(self.bucket, op=dist.ReduceOp.SUM, group=self.group)
            elif self.has_group:
                if self.gathered is None:
                    self.gathered = torch.empty((self.world, self.total), dtype=torch.float32, device=self.device)
                if self.backend == "nccl":
                    dist.all_gather_into_tensor(self.gathered, self.bucket, group=self.group)
                else:                                                      # (gloo: the list form)
                    dist.all_gather(list(self.gathered.unbind(0)), self.bucket, group=self.group)
                hip.opt_reduce_ranks(self.gathered, self.bucket)
        for p, v in zip(self.params, self.views):
            p.grad = v

    @torch.no_grad()
    def broadcast_parameters(self, src=0, buffers=()):
        """Every parameter handed to the constructor (frozen ones too) and every tensor of ``buffers`` := rank ``src``'s: one pack, one
        ``dist.broadcast``, one unpack over the fp32 tensors (any other dtype is broadcast on its own), and a move of the version counters
        of what was written, on which the packed-operand caches are keyed.  Without a process group there is nothing to do."""
        if not self.has_group:
            return
        tensors = [p for _, p in self.all_named] + [b for b in buffers]
        flat = [t for t in tensors if t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device and t.numel()]
        chosen = {id(t) for t in flat}
        if flat:
            entries = [(t.data_ptr(), t.data_ptr(), t.numel()) for t in flat]                # (pack reads g, unpack writes p: the same tensor)
            tables = hip.BucketTables(entries, self.device)
            wire = torch.empty(tables.total, dtype=torch.float32, device=self.device)
            hip.opt_pack_grads(tables, wire, 1.0)
            dist.broadcast(wire, src, group=self.group)
            hip.opt_unpack_grads(tables, wire)
        for t in tensors:
            if id(t) not in chosen and t.numel():
                own = t.detach().contiguous()
                dist.broadcast(own, src, group=self.group)
                t.detach().copy_(own)
        torch.autograd.graph.increment_version(tensors)
