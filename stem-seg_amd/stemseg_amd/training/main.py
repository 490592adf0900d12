"""The training loop under the reference's names (training/main.py): ``Trainer(cfg, model_save_dir, args, logger)`` with ``start``,
``backup_session`` and ``restore_session``, and the command line of ``python -m stemseg_amd.training.main`` with the reference's flags.

One optimiser step is fed by ``optimizer_step_interval`` sub-iterations: each runs the model on one batch and back-propagates its summed
optimisation losses divided by that interval, so the gradients accumulate to the mean over the whole batch; then come the step, the
scheduler's step and ``zero_grad``.  A checkpoint holds the keys 'model', 'optimizer', 'lr_scheduler', 'logger' and 'iterations', as the
reference's do, so either side resumes the other's sessions.

Data-parallel training is opt-in, like every other training switch: ``Trainer(..., data_parallel=True)`` on an initialised process group,
or ``--allow_multigpu`` on the command line with more than one visible device (the reference's launcher contract: one process per GPU,
``--local_rank`` the rank and the device, ``--master_port`` the rendezvous).  Every rank then starts from rank 0's parameters and buffers,
runs ``optimizer_step_interval(..., num_gpus)`` sub-iterations on its own batches with no communication (what DistributedDataParallel's
``no_sync`` buys), and ``optimizer_step`` first averages the gradients over the ranks through a ``GradBucket`` -- one pack launch and one
collective, after a rebuild of its small tables on the host when the gradients' addresses have moved -- so that the clip's norm and coefficient and the step are bit-identical on every rank.  The logged means are reduced to rank
0, and only rank 0 logs, writes and prunes checkpoints.  A signal is looked at by all ranks together, once per step (``any_rank``); a
rank that fails saves nothing and waits for nobody, rank 0 writes its emergency checkpoint alone (``emergency_backup``), and the other
ranks then end in the group's timeout at their next collective.  Out of scope: the sampler (a caller shards its data with
``torch.utils.data.distributed.DistributedSampler``), overlap of the communication with the backward pass, and mixed precision.

What differs from the reference, on purpose:
  * without ``data_parallel`` an initialised process group of more than one rank is refused; with it the gradients are averaged by
    ``GradBucket`` at the step, not by DistributedDataParallel's hooks during the backward pass;
  * TRAINING.MIXED_PRECISION is refused (the reference hands it to apex);
  * ``configure_trainable`` maps TRAINING.FREEZE_BACKBONE / MODEL.BACKBONE.FREEZE_AT_STAGE onto ``requires_grad`` and the model's switches;
  * TRAINING.CLIP_GRADIENTS, a key the reference defines and never reads, clips the global gradient norm at ``max_norm`` (10.0) on the device:
    ``grad_norm`` leaves the coefficient in device memory and the step kernel applies it, so clipping costs no read-back;
  * outdated checkpoints are really pruned (the reference's glob pattern matches no file);
  * the data loader is the caller's by default: any iterable of ``(image_seqs, targets, meta_info)``, handed to
    ``start(args, cfg, data_loader)``.  --build_data_loader makes the session build the reference's own from ``stemseg_amd.data``: the
    video datasets of the preset, their batches put together on the device (``data.common.device_collate``).
"""
import argparse
import glob
import logging
import os
import signal
import time

import torch
import torch.distributed as dist

from .. import config as _config
from ..modeling.model_builder import build_model
from ..utils.paths import ModelPaths
from .model_output_manager import ModelOutputManager
from ..utils import distributed as dist_utils
from .optim import DeviceAdam, DeviceSGD, GradBucket, grad_norm
from .utils import (configure_trainable, create_lr_scheduler, create_optimizer, create_training_data_loader, create_training_dataset,
                    optimizer_step_interval, register_log_level_type, var_keys_to_str)

CHECKPOINT_KEYS = ("model", "optimizer", "lr_scheduler", "logger", "iterations")


class InterruptException(RuntimeError):
    """SIGINT or SIGTERM arrived while the loop ran."""


class InterruptDetector(object):
    """While started, SIGINT and SIGTERM only raise ``is_interrupted``; the loop looks at it between sub-iterations, so a session is
    never cut inside a step.  ``stop`` puts the earlier handlers back.  Outside the main thread no handler can be installed: idle there."""

    def __init__(self):
        self.is_interrupted = False
        self._earlier = {}

    def start(self):
        def note(signum, frame):
            self.is_interrupted = True
        try:
            for sig in (signal.SIGINT, signal.SIGTERM):
                self._earlier[sig] = signal.signal(sig, note)
        except ValueError:
            pass

    def stop(self):
        while self._earlier:
            sig, handler = self._earlier.popitem()
            signal.signal(sig, handler)


class TrainingLogger(object):
    """The clock of a session and its scalar log.  ``state_dict`` uses the keys of the reference's TrainingLogger (its name-mangled
    private attributes), which is what its checkpoints hold under 'logger'.  Scalars go to a tensorboardX writer where that package is
    installed; the last point is always kept in ``last_point``."""

    _KEYS = {"started": "_TrainingLogger__train_start_time", "latest": "_TrainingLogger__latest_timestamp",
             "iteration": "_TrainingLogger__latest_iteration_num", "paused": "_TrainingLogger__pause_duration"}

    def __init__(self, output_dir, num_iterations=None):
        os.makedirs(output_dir, exist_ok=True)
        self.output_dir, self.total_iterations = output_dir, num_iterations
        self.started = self.latest = self.iteration = None
        self.paused = 0.0
        self.last_point = {}
        self.last_validation = {}
        try:
            import tensorboardX
            self.writer = tensorboardX.SummaryWriter(output_dir)
        except ImportError:
            self.writer = None

    def start_timer(self):
        """Start the clock, or -- a resumed session -- book the time since the last logged point as a pause."""
        now = time.time()
        if self.started is None or self.iteration is None:
            self.started = now
        else:
            self.paused += now - self.latest

    def add_training_point(self, iteration_num, add_to_summary, **scalars):
        self.latest, self.iteration = time.time(), iteration_num
        self.last_point = dict(scalars, iteration=iteration_num)
        if add_to_summary and self.writer is not None:
            for name, value in scalars.items():
                self.writer.add_scalar("training_" + name, value, iteration_num)

    def add_validation_point(self, iteration_num, **scalars):
        """The figures of one ``validate_fn`` call: ``validation_<name>`` scalars, kept in ``last_validation``; the clock is not touched."""
        self.last_validation = dict(scalars, iteration=iteration_num)
        if self.writer is not None:
            for name, value in scalars.items():
                self.writer.add_scalar("validation_" + name, value, iteration_num)

    def compute_eta(self, as_string=True):
        """-> (time left, seconds per iteration so far), pauses not counted; the time as 'd-hh:mm:ss' or in seconds."""
        if self.started is None or self.latest is None:
            raise RuntimeError("TrainingLogger.compute_eta before the first training point")
        per_iteration = (self.latest - self.started - self.paused) / self.iteration
        left = (self.total_iterations - self.iteration) * per_iteration
        if as_string:
            m, s = divmod(int(left), 60)
            h, m = divmod(m, 60)
            d, h = divmod(h, 24)
            left = "%d-%02d:%02d:%02d" % (d, h, m, s)
        return left, per_iteration

    def state_dict(self):
        return dict({key: getattr(self, attr) for attr, key in self._KEYS.items()}, total_iterations=self.total_iterations)

    def load_state_dict(self, state):
        attrs = dict({key: attr for attr, key in self._KEYS.items()}, total_iterations="total_iterations")
        unknown = sorted(set(state) - set(attrs))
        if unknown:
            raise KeyError("TrainingLogger.load_state_dict: unknown keys %s" % unknown)
        for key, value in state.items():
            setattr(self, attrs[key], value)


def _to_device(x, device):
    """Tensors of a nested dict / list / tuple structure (and anything else with a ``.to``) moved to ``device``."""
    if torch.is_tensor(x) or (hasattr(x, "to") and not isinstance(x, (str, bytes))):
        return x.to(device=device)
    if isinstance(x, dict):
        return {k: _to_device(v, device) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_device(v, device) for v in x)
    return x


class Trainer(object):
    """cfg: the TRAINING section of the global cfg.  args: restore_session, initial_ckpt (paths or None).  model: a ``TrainingModel``
    (default: ``build_model(restore_pretrained_backbone_wts=True)``); data_loader: an iterable of ``(image_seqs, targets, meta_info)``.
    max_norm: the clip threshold of TRAINING.CLIP_GRADIENTS.  device_step: the optimiser on csrc/optimizer.hip (False: the stock classes).
    data_parallel: train on every rank of the default process group, the gradients averaged by a ``GradBucket`` in ``reduce_mode``
    ("allreduce" | "ordered") before each step; without a group it runs the same path on one GPU.
    validate_fn: opt-in; ``validate_fn(trainer)`` -> {name: float}, called by ``start`` on the main process every
    ``opts.validation_interval`` optimiser steps (``validate``)."""

    def __init__(self, cfg, model_save_dir, args, logger, model=None, data_loader=None, max_norm=10.0, device_step=True, data_parallel=False,
                 reduce_mode="allreduce", validate_fn=None):
        if not data_parallel and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("Trainer: a process group of %d ranks is initialised, and without data_parallel=True neither "
                                      "DistributedDataParallel nor the gradient all-reduce is run: pass data_parallel=True, or train on one GPU"
                                      % dist.get_world_size())
        if reduce_mode not in GradBucket.MODES:
            raise ValueError("Trainer: reduce_mode %r is not one of %s" % (reduce_mode, GradBucket.MODES))
        if cfg.MIXED_PRECISION:
            raise NotImplementedError("TRAINING.MIXED_PRECISION: the reference hands mixed precision to apex (apex.amp), which this library does "
                                      "not use; the kernels and the optimiser step are fp32")
        if args.restore_session is not None and args.initial_ckpt is not None:
            raise ValueError("Trainer: restore_session and initial_ckpt exclude each other")
        self.cfg, self.console_logger, self.model_save_dir = cfg, logger, model_save_dir
        self.data_parallel = bool(data_parallel)
        if self.data_parallel:
            self.num_gpus, self.local_rank, self.is_main_process = dist_utils.get_world_size(), dist_utils.get_rank(), dist_utils.is_main_process()
        else:
            self.num_gpus, self.local_rank, self.is_main_process = 1, 0, True
        self.local_device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.log_dir = os.path.join(model_save_dir, "logs")
        if model is None:
            model = build_model(restore_pretrained_backbone_wts=True, logger=logger)
        # (args.train_stem, --train_stem: MODEL.BACKBONE.FREEZE_AT_STAGE 0 and 1 train layer1 and the stem, csrc/stem_backward.hip)
        stem = {"train_stem": True} if getattr(args, "train_stem", False) else {}
        self.model = configure_trainable(model.to(self.local_device), freeze_backbone=cfg.FREEZE_BACKBONE, **stem)
        self.optimizer = create_optimizer(self.model, cfg, logger.info, device_step=device_step)
        self.lr_scheduler = create_lr_scheduler(self.optimizer, cfg, logger.info)
        self.logger = TrainingLogger(self.log_dir) if self.is_main_process else None          # (the other ranks keep no clock and write no file)
        self.interrupt_detector = InterruptDetector()
        self.data_loader = data_loader
        self.max_norm = float(max_norm)
        self.validate_fn = validate_fn
        self.total_iterations, self.elapsed_iterations = cfg.MAX_ITERATIONS, 0
        self.last_grad_norm = None          # device float64 [1] of the last clipped step
        read = lambda path: torch.load(path, map_location=self.local_device)
        if args.restore_session is not None:
            logger.info("resuming the session saved in %s" % args.restore_session)
            self.restore_session(read(args.restore_session))
        elif args.initial_ckpt is not None:
            logger.info("starting from the model weights in %s" % args.initial_ckpt)
            self.model.load_state_dict(read(args.initial_ckpt)["model"])
        self.bucket = None
        if self.data_parallel:
            self.bucket = GradBucket(self.model.named_parameters(), mode=reduce_mode)
            self.bucket.broadcast_parameters(0, buffers=self.model.buffers())

    @property
    def _model(self):
        return self.model

    def backup_session(self):
        """Write <model_save_dir>/<iterations, six digits>.pth and return its path.  Data-parallel: a COLLECTIVE -- rank 0 alone writes,
        between two barriers, as in the reference's regular save; the other ranks return None.  Every rank must call it at the same
        point of the loop; a rank that has failed calls ``emergency_backup`` instead."""
        if self.data_parallel:
            dist_utils.synchronize()
            path = self._write_session() if self.is_main_process else None
            dist_utils.synchronize()
            return path
        return self._write_session()

    def emergency_backup(self):
        """The save of a session that is about to end in an error, as in the reference's failure path: the main process writes, alone and
        with no collective -- the other ranks may be anywhere, inside the gradient reduction included, and a barrier here would be
        matched against whatever they are in.  -> the path, or None on the other ranks."""
        return self._write_session() if self.is_main_process else None

    def _write_session(self):
        parts = {"model": self._model, "optimizer": self.optimizer, "lr_scheduler": self.lr_scheduler, "logger": self.logger}
        session = {key: part.state_dict() for key, part in parts.items()}
        session["iterations"] = self.elapsed_iterations
        path = os.path.join(self.model_save_dir, "%06d.pth" % self.elapsed_iterations)
        torch.save(session, path)
        self.console_logger.info("session saved to %s" % path)
        return path

    def restore_session(self, restore_dict):
        missing = [key for key in CHECKPOINT_KEYS if key not in restore_dict]
        if missing:
            raise KeyError("restore_session: the checkpoint lacks %s" % missing)
        for key, part in (("model", self._model), ("optimizer", self.optimizer), ("lr_scheduler", self.lr_scheduler), ("logger", self.logger)):
            if part is not None:
                part.load_state_dict(restore_dict[key])
        self.elapsed_iterations = restore_dict["iterations"]

    def prune_checkpoints(self, ckpts_to_keep):
        """Remove all but the newest ``ckpts_to_keep`` of the numbered checkpoints."""
        numbered = sorted(glob.glob(os.path.join(self.model_save_dir, "[0-9]" * 6 + ".pth")))
        for path in numbered[:max(0, len(numbered) - int(ckpts_to_keep))]:
            os.remove(path)

    def optimizer_step(self):
        """The step, with the clip when TRAINING.CLIP_GRADIENTS; then the scheduler and ``zero_grad``.  Data-parallel: the gradients are
        averaged over the ranks first, so the norm, the coefficient and the step are the same on every rank."""
        if self.bucket is not None:
            self.bucket.reduce()
        if not self.cfg.CLIP_GRADIENTS:
            self.optimizer.step()
        elif isinstance(self.optimizer, (DeviceSGD, DeviceAdam)):
            self.last_grad_norm, coef, _ = grad_norm(self.model.parameters(), self.max_norm)
            self.optimizer.step(grad_scale=coef)
        else:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_norm).double().reshape(1)
            self.optimizer.step()
        self.lr_scheduler.step()
        self.optimizer.zero_grad()
        self.elapsed_iterations += 1

    def validate(self):
        """Call ``validate_fn(trainer)`` on the main process under ``torch.no_grad()`` and log the dict of floats it returns as
        ``validation_<key>`` scalars.  Data-parallel: a COLLECTIVE, like ``backup_session`` -- the main process validates between two
        barriers while the other ranks wait.  -> the figures (None on the other ranks)."""
        if self.data_parallel:
            dist_utils.synchronize()
        values = None
        if self.is_main_process:
            with torch.no_grad():
                values = {k: float(v) for k, v in self.validate_fn(self).items()}
            self.logger.add_validation_point(self.elapsed_iterations, **values)
            self.console_logger.info("iteration %05d | validation | %s" % (self.elapsed_iterations, " - ".join("%s: %.4f" % kv for kv in values.items())))
        if self.data_parallel:
            dist_utils.synchronize()
        return values

    def _log_iteration(self, means, opts):
        if self.data_parallel:
            means = dist_utils.reduce_dict(means)          # (a collective: every rank takes part, rank 0 holds the means)
        if not self.is_main_process:
            return
        values = {k: v.item() for k, v in means.items()}
        if self.cfg.CLIP_GRADIENTS:
            values["grad_norm"] = float(self.last_grad_norm)
        it = self.elapsed_iterations
        self.logger.add_training_point(it, it % opts.summary_interval == 0, **values)
        values["lr"] = self.lr_scheduler.get_last_lr()[0]
        eta, per_iteration = self.logger.compute_eta()
        say = self.console_logger.info if it % opts.display_interval == 0 else self.console_logger.debug
        say("iteration %05d | %s | %.3f s per iteration, %s to go" % (it, var_keys_to_str(values), per_iteration, eta))

    def start(self, opts):
        """Run over the data loader until it ends or TRAINING.MAX_ITERATIONS optimiser steps are done.  opts: display_interval,
        summary_interval, save_interval, ckpts_to_keep, and optionally validation_interval (0 or absent: never; else ``validate`` runs
        every so many optimiser steps when the Trainer has a ``validate_fn``)."""
        if self.data_loader is None:
            raise ValueError("Trainer.start: no data loader; pass data_loader=, an iterable of (image_seqs, targets, meta_info), or run "
                             "the command line with --build_data_loader")
        interval, _ = optimizer_step_interval(self.cfg.BATCH_SIZE, self.cfg.MAX_SAMPLES_PER_GPU, self.cfg.ACCUMULATE_GRADIENTS, self.num_gpus)
        say = self.console_logger.info if self.is_main_process else self.console_logger.debug
        say(
            "training from iteration %d to %d: batch size %d, an optimiser step every %d sub-iterations, %d trainable values, a checkpoint "
            "every %d iterations in %s" % (self.elapsed_iterations, self.total_iterations, self.cfg.BATCH_SIZE, interval,
                                           sum(p.numel() for p in self.model.parameters() if p.requires_grad), opts.save_interval,
                                           self.model_save_dir))
        if self.logger is not None:
            self.logger.total_iterations = self.total_iterations
            self.logger.start_timer()
        outputs = ModelOutputManager(interval)
        validation_interval = int(getattr(opts, "validation_interval", 0) or 0) if self.validate_fn is not None else 0
        pending = 0                          # sub-iterations whose gradients wait for the step
        self.interrupt_detector.start()
        try:
            for image_seqs, targets, _meta_info in self.data_loader:
                if self.interrupt_detector.is_interrupted and not self.data_parallel:
                    raise InterruptException()
                loss = outputs(self.model(_to_device(image_seqs, self.local_device), _to_device(targets, self.local_device)))
                loss.backward()
                pending += 1
                if pending < interval:
                    continue
                pending = 0
                self.optimizer_step()
                self._log_iteration(outputs.reset()[0], opts)
                done = self.elapsed_iterations
                if done % opts.save_interval == 0:
                    self.backup_session()
                    if self.is_main_process:
                        self.prune_checkpoints(opts.ckpts_to_keep)
                if validation_interval > 0 and done % validation_interval == 0:
                    self.validate()
                # data-parallel: the ranks look at the signal together, at the step, so that all of them leave the loop at the same
                # iteration and none is left waiting in the next reduction for a rank that has gone
                if self.data_parallel and dist_utils.any_rank(self.interrupt_detector.is_interrupted):
                    raise InterruptException()
                if done >= self.total_iterations:
                    break
        finally:
            self.interrupt_detector.stop()
        say("training ended at iteration %d; checkpoints in %s, logs in %s"
                                 % (self.elapsed_iterations, self.model_save_dir, self.log_dir))


def create_logger(args):
    """The console logger of a session: time, level and message on the stream, at ``args.log_level``."""
    logger = logging.getLogger("stemseg_amd.training")
    logger.setLevel(args.log_level)
    logger.propagate = False
    if not logger.handlers:
        handler = logging.StreamHandler()
        handler.setFormatter(logging.Formatter("%(asctime)s %(levelname)s %(message)s", "%H:%M:%S"))
        logger.addHandler(handler)
    return logger


def build_data_loader(trainer, args):
    """The reference's loader for a session (training/main.py:138, 179-181): the dataset mix of the preset over MAX_ITERATIONS x BATCH_SIZE
    samples, shuffled, in batches of what one sub-iteration takes, skipping the iterations a resumed session has done.  The datasets are
    read from the STEMSEG_JSON_ANNOTATIONS_DIR / *_BASE_DIR paths of ``utils/paths.py``."""
    cfg = trainer.cfg
    device_augmentation = bool(getattr(args, "device_augmentation", False))
    device_mapillary = bool(getattr(args, "device_mapillary", False))
    dataset = create_training_dataset(trainer.total_iterations * cfg.BATCH_SIZE, print_fn=trainer.console_logger.info,
                                      mode=_config.PRESET_TRAINING_MODES.get(args.cfg), device_augmentation=device_augmentation,
                                      device_mapillary=device_mapillary)
    _, per_sub_iteration = optimizer_step_interval(cfg.BATCH_SIZE, cfg.MAX_SAMPLES_PER_GPU, cfg.ACCUMULATE_GRADIENTS, trainer.num_gpus)
    return create_training_data_loader(dataset, per_sub_iteration, True, None, args.num_cpu_workers, trainer.elapsed_iterations,
                                       device_augmentation=device_augmentation, device_mapillary=device_mapillary)


def start(args, cfg, data_loader=None, data_parallel=False, validate_fn=None):
    """One session in <STEMSEG_MODELS_DIR>/checkpoints/<TRAINING.MODE>/<--model_dir>.  The newest checkpoint found there is resumed from
    unless --no_resume; when the loop is interrupted or fails, the session is saved before the error travels on.  With
    --build_data_loader and no ``data_loader``, the session builds its own (``build_data_loader``) once it knows where it resumes."""
    logger = create_logger(args)
    save_dir = os.path.join(ModelPaths.checkpoint_base_dir(), cfg.MODE, args.model_dir)
    os.makedirs(save_dir, exist_ok=True)
    saved = sorted(glob.glob(os.path.join(save_dir, "*.pth")))
    if saved and not args.no_resume:
        args.restore_session, args.initial_ckpt = saved[-1], None
    trainer = Trainer(cfg, save_dir, args, logger, data_loader=data_loader, data_parallel=data_parallel, validate_fn=validate_fn)
    if data_loader is None and getattr(args, "build_data_loader", False):
        trainer.data_loader = build_data_loader(trainer, args)
    try:
        trainer.start(args)
    except (Exception, KeyboardInterrupt) as err:
        logger.error("%s: saving the session before giving up" % type(err).__name__)
        trainer.emergency_backup()
        raise


def build_parser():
    """The reference's command line (training/main.py): same flags, same defaults."""
    parser = argparse.ArgumentParser(description="train a STEm-Seg model on one MI355X")
    level = register_log_level_type(parser)
    for flag in ("--model_dir", "--cfg"):
        parser.add_argument(flag, type=str, required=True)
    for flag in ("--restore_session", "--initial_ckpt"):
        parser.add_argument(flag, type=str, required=False)
    for flag in ("--no_resume", "--allow_multigpu", "--build_data_loader"):          # (--build_data_loader: this library's opt-in, see main)
        parser.add_argument(flag, action="store_true")
    # with --build_data_loader: the COCO / Pascal VOC image datasets and the instance duplicator, warped on the device (csrc/augment.hip)
    parser.add_argument("--device_augmentation", action="store_true")
    # with --build_data_loader: the Mapillary image dataset of the kitti_mots mix (kittimots_1), warped and its ignore mask built on the device
    parser.add_argument("--device_mapillary", action="store_true")
    # MODEL.BACKBONE.FREEZE_AT_STAGE 0 and 1: the backward of layer1, the max-pool and the stem's 7x7 convolution (csrc/stem_backward.hip)
    parser.add_argument("--train_stem", action="store_true")
    for flag, default in (("--local_rank", 0), ("--master_port", "12356"), ("--display_interval", 5), ("--summary_interval", 10),
                          ("--save_interval", 10000), ("--num_cpu_workers", 8), ("--ckpts_to_keep", 2),
                          ("--validation_interval", 0)):          # (--validation_interval: this library's; it acts on a Trainer with a validate_fn)
        parser.add_argument(flag, type=type(default), default=default)          # (the two multi-GPU flags: init_distributed, under --allow_multigpu)
    parser.add_argument("--log_level", type=level, default=logging.INFO)
    parser.add_argument("--subprocess_log_level", type=level, default=logging.WARN)
    return parser


def init_distributed(args, num_gpus):
    """The reference's launcher contract (training/main.py): one process per GPU, each started with its ``--local_rank``; rank and device
    are that number, the rendezvous is 127.0.0.1 (or a MASTER_ADDR already set) at ``--master_port``, the backend nccl."""
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(args.master_port)
    torch.cuda.set_device(args.local_rank)
    dist.init_process_group("nccl", rank=args.local_rank, world_size=num_gpus, device_id=torch.device("cuda", args.local_rank))


def main(args, data_loader=None, validate_fn=None):
    """--cfg: a preset name of ``stemseg_amd.config`` (davis | davis_2 | ytvis | kittimots | kittimots_1).  data_loader: the iterable to train on.  The
    command line alone has none: ``python -m stemseg_amd.training.main`` checks the configuration, builds the Trainer and stops at
    ``Trainer.start`` asking for one -- unless --build_data_loader, with which the session builds the preset's dataset mix and its loader
    (``build_data_loader``; under --allow_multigpu sharded by the ``DistributedSampler`` port) and trains on it.
    --allow_multigpu with more than one visible device: this process is
    rank --local_rank of as many ranks as there are devices, and trains data-parallel; with one device the flag is ignored, as in the
    reference.  validate_fn: handed to the Trainer, which calls it every --validation_interval optimiser steps (0: never)."""
    if getattr(args, "device_augmentation", False) and not getattr(args, "build_data_loader", False):
        raise ValueError("--device_augmentation configures the loader that --build_data_loader builds: pass both")
    if getattr(args, "device_mapillary", False) and not getattr(args, "build_data_loader", False):
        raise ValueError("--device_mapillary configures the loader that --build_data_loader builds: pass both")
    num_gpus = torch.cuda.device_count()
    data_parallel = bool(args.allow_multigpu) and num_gpus > 1
    _config.load_preset(args.cfg)
    extra = {} if validate_fn is None else {"validate_fn": validate_fn}
    if not data_parallel:
        return start(args, _config.cfg.TRAINING, data_loader, **extra)
    init_distributed(args, num_gpus)
    try:
        start(args, _config.cfg.TRAINING, data_loader, data_parallel=True, **extra)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(build_parser().parse_args())
