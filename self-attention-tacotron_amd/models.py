"""Model plugin surface: encoder / decoder / model factories and ``model_fn``.

Mirrors models/models.py:20-378: ``encoder_factory(params, is_training)``,
``decoder_factory(params)``, ``tacotron_model_factory(hparams, model_dir, run_config,
warm_start_from=None)`` keyed by the ``hparams.encoder`` / ``decoder`` / ``tacotron_model``
strings (unknown -> ``ValueError``, as the reference), and the Estimator-shaped
``DualSourceSelfAttentionTacotronModel`` whose ``model_fn(features, labels, mode, params)``
returns an ``EstimatorSpec``:

* TRAIN  -- one full training step on libsat_hip (masks drawn on the device, forward, BPTT,
  [RCCL all-reduce], clip_by_global_norm(1.0) + TF Adam + Noam decay), loss = 0.1 L1 + BCE
  (models/models.py:151-189);
* EVAL   -- ``loss`` of the validation decode (OneHotValidationHelper: softmax feedback, exactly
  T' steps with real attention; models/models.py:86-97) plus the teacher-forced
  ``loss_with_teacher`` metrics (models/models.py:208-235, 305-320); eval semantics (dropout off,
  zoneout blend, BatchNorm moving statistics), except that ``apply_dropout_on_inference`` keeps
  the decoder prenets' dropout on in EVAL and PREDICT (inference.py);
* PREDICT -- free-running inference (BASELINE configs[4]; inference.FreeRunningDecoder: the
  stop-token helper + the KV-cached incremental decoder self-attention), returning the
  reference's predictions dict (models/models.py:252-277).

``features`` / ``labels`` follow the reference's dataset records (``PreprocessedSourceData`` /
``PreprocessedTargetData``, datasets/codes/dataset.py:45-48; ``codes`` is the mel target for
LJSpeech/VCTK), as device tensors or numpy arrays.
"""

from __future__ import annotations

import os
from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import torch

from . import checkpoint as C
from . import dp
from . import params as PR
from .engine import Tacotron
from .train import StepGraphCache, Trainer


class ModeKeys:
    """tf.estimator.ModeKeys values."""
    TRAIN = "train"
    EVAL = "eval"
    PREDICT = "infer"


PreprocessedSourceData = namedtuple(
    "PreprocessedSourceData", ["id", "key", "source", "source_length", "text"])
PreprocessedTargetData = namedtuple(
    "PreprocessedTargetData", ["id", "key", "codes", "target_length", "done", "code_loss_mask",
                               "binary_loss_mask"])
# VCTK records (datasets/vctk/dataset.py:31-46): source carries speaker_id / age / gender, and
# the target is MelData with spec_loss_mask in place of code_loss_mask.
SourceData = namedtuple(
    "SourceData", ["id", "key", "source", "source_length", "speaker_id", "age", "gender", "text"])
MelData = namedtuple(
    "MelData", ["id", "key", "mel", "mel_width", "target_length", "done", "spec_loss_mask",
                "binary_loss_mask"])
EstimatorSpec = namedtuple("EstimatorSpec", ["mode", "loss", "train_op", "predictions",
                                             "eval_metric_ops"])
# tf.estimator.WarmStartSettings as train.py:75-77 builds it: a checkpoint (file, or a directory
# whose newest checkpoint is taken) and the regexes of the variables to initialise from it
WarmStartSettings = namedtuple("WarmStartSettings",
                               ["ckpt_to_initialize_from", "vars_to_warm_start"],
                               defaults=((".*",),))


class SelfAttentionCBHGEncoder:
    """Configuration of modules/module.py:378-438 as built by encoder_factory
    (models/models.py:325-346); executed by libsat_hip inside the model step."""

    def __init__(self, is_training, **cfg):
        self.is_training = is_training
        self.config = cfg


class DualSourceTransformerDecoder:
    """Configuration of modules/module.py:1455-1562 as built by decoder_factory
    (models/models.py:349-368)."""

    def __init__(self, **cfg):
        self.config = cfg


def encoder_factory(params, is_training):
    if params.encoder == "SelfAttentionCBHGEncoder":
        return SelfAttentionCBHGEncoder(
            is_training, cbhg_out_units=params.cbhg_out_units,
            conv_channels=params.conv_channels, max_filter_width=params.max_filter_width,
            projection1_out_channels=params.projection1_out_channels,
            projection2_out_channels=params.projection2_out_channels,
            num_highway=params.num_highway,
            self_attention_out_units=params.self_attention_out_units,
            self_attention_num_heads=params.self_attention_num_heads,
            self_attention_num_hop=params.self_attention_num_hop,
            prenet_out_units=params.encoder_prenet_out_units,
            drop_rate=params.encoder_prenet_drop_rate,
            zoneout_factor_cell=params.zoneout_factor_cell,
            zoneout_factor_output=params.zoneout_factor_output,
            self_attention_drop_rate=params.self_attention_drop_rate)
    raise ValueError(f"Unknown encoder: {params.encoder}")


def decoder_factory(params):
    if params.decoder == "DualSourceTransformerDecoder":
        return DualSourceTransformerDecoder(
            prenet_out_units=params.decoder_prenet_out_units,
            drop_rate=params.decoder_prenet_drop_rate,
            attention_rnn_out_units=params.attention_out_units,
            decoder_version=params.decoder_version, decoder_out_units=params.decoder_out_units,
            num_mels=params.num_mels, outputs_per_step=params.outputs_per_step,
            max_iters=params.max_iters, n_feed_frame=params.n_feed_frame,
            zoneout_factor_cell=params.zoneout_factor_cell,
            zoneout_factor_output=params.zoneout_factor_output,
            self_attention_out_units=params.decoder_self_attention_out_units,
            self_attention_num_heads=params.decoder_self_attention_num_heads,
            self_attention_num_hop=params.decoder_self_attention_num_hop,
            self_attention_drop_rate=params.decoder_self_attention_drop_rate)
    raise ValueError(f"Unknown decoder: {params.decoder}")


def _to_device(x, dev, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype)
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=dev)


class _PinnedStager:
    """Host -> device upload of a batch without a host-side wait.  A pageable ``as_tensor(...,
    device=)`` blocks the host until the stream has drained (a synchronous copy), so the next
    step's launches only start once the GPU is idle.  Here each array is packed into a pinned
    buffer and copied with ``non_blocking=True`` in stream order; buffers rotate over a small
    ring and a slot is rewritten only after the copy that last read it has finished (its event),
    so the host runs ahead of the device by up to ``depth`` batches."""

    def __init__(self, depth: int = 3):
        self.depth = depth
        self.slots = [dict() for _ in range(depth)]     # name -> pinned uint8 buffer
        self.events = [None] * depth
        self.i = 0

    def upload(self, arrays, dev, dtypes):
        """arrays: name -> numpy / tensor; dtypes: name -> torch dtype.  Returns device tensors."""
        if not torch.cuda.is_available() or torch.device(dev).type != "cuda":
            return {k: _to_device(v, dev, dtypes[k]) for k, v in arrays.items()}
        slot, ev = self.slots[self.i], self.events[self.i]
        if ev is not None:
            ev.synchronize()                             # that slot's last copy is done
        out = {}
        for k, v in arrays.items():
            if isinstance(v, torch.Tensor) and v.is_cuda:
                out[k] = v.to(dtype=dtypes[k])
                continue
            h = torch.as_tensor(np.ascontiguousarray(np.asarray(v))).to(dtypes[k])
            nb = h.numel() * h.element_size()
            buf = slot.get(k)
            if buf is None or buf.numel() < nb:
                buf = torch.empty(max(nb, 1), dtype=torch.uint8, pin_memory=True)
                slot[k] = buf
            pin = buf[:nb].view(h.dtype).view(h.shape)
            pin.copy_(h)
            out[k] = torch.empty(h.shape, dtype=h.dtype, device=dev)
            out[k].copy_(pin, non_blocking=True)
        e = torch.cuda.Event()
        e.record()
        self.events[self.i] = e
        self.i = (self.i + 1) % self.depth
        return out


class DualSourceSelfAttentionTacotronModel:
    """Estimator-shaped model (models/models.py:20-320) over the libsat_hip engine."""

    def __init__(self, params, model_dir=None, config=None, warm_start_from=None,
                 device="cuda", seed: int = 1234,
                 init_values: Optional[Dict[str, np.ndarray]] = None,
                 graph_cache: Optional[int] = None, graph_t_quantum: Optional[int] = None,
                 summaries: bool = False):
        """``summaries`` (with a ``model_dir``): TRAIN writes TensorBoard scalars every
        ``save_summary_steps`` steps and, under ``save_training_time_metrics``, alignment / mel
        images every ``alignment_save_steps`` steps into ``model_dir``; ``evaluate()`` writes
        its metrics and images into ``model_dir/eval`` (summary.py).  Off by default: no event
        file and no extra launch.

        ``graph_cache``: captured training steps kept per padded batch shape (LRU; 0 = every
        TRAIN step eager; default SAT_GRAPH_CACHE or 0); ``graph_t_quantum``: pad T' to a
        multiple of it before the lookup (default SAT_GRAPH_T_QUANTUM or 0 = exact shapes;
        train.StepGraphCache).  Default eager: with the pinned asynchronous upload the eager
        drop-in path keeps the GPU busy (its host issue runs ahead of the device), and it
        measured as fast as the cache's steady state over ragged LJSpeech-like batches (bench
        ``drop_in_ragged_ljs``), without the cache's first-sighting capture cost."""
        encoder_factory(params, True)                        # name checks, as the reference
        if params.decoder not in ("DualSourceDecoder", "DualSourceTransformerDecoder"):
            raise AssertionError(f"decoder must be a dual-source decoder: {params.decoder}")
        decoder_factory(params)
        if params.use_speaker_embedding and params.use_external_speaker_embedding:
            raise AssertionError("only one of speaker_embedding / external_speaker_embedding")
        PR.resolve_dims(params)                              # shapes this build supports
        self.params = params
        self.model_dir = model_dir
        self.config = config
        self.engine = Tacotron(params, device, seed=seed, init_values=init_values)
        self._pending = None                 # a restored checkpoint whose optimiser state waits
        self._state_path = None              # the file the current state equals (None: trained on)
        self._host_step = 0
        self._pending_rank0_only = False
        # rank 0's view of model_dir decides for every replica (ONE broadcast every rank enters)
        newest = dp.from_rank0(C.latest_checkpoint(model_dir) if model_dir else None)
        if warm_start_from is not None and newest is None:
            # as an Estimator: warm start only where model_dir holds no checkpoint to resume
            self._warm_start(warm_start_from)
        # data-parallel replicas start from rank 0's weights and statistics
        dp.broadcast_params(self.engine.params)
        dp.broadcast_params(self.engine.bn.buf)
        self._trainer: Optional[Trainer] = None
        self._graphs: Optional[StepGraphCache] = None
        self._stager = _PinnedStager()
        env = os.environ.get
        self.graph_cache = int(env("SAT_GRAPH_CACHE", "0") if graph_cache is None else graph_cache)
        self.graph_t_quantum = int(env("SAT_GRAPH_T_QUANTUM", "0") if graph_t_quantum is None
                                   else graph_t_quantum)
        # dropout / zoneout masks differ per replica (each rank's shard is its own batch)
        self._seed_offset = 1000003 * dp.rank()
        self._seed = seed + self._seed_offset
        self._eval_decoder = None
        # apply_dropout_on_inference: the device seed word of every prenet mask drawn outside
        # training (PREDICT / EVAL decodes and the teacher-forced eval passes share it; each
        # draw advances it).  Starts from this replica's seed; not part of a checkpoint.
        self._infer_seed_dev = None
        # event files: rank 0 alone writes (no other rank queues, launches or communicates)
        self.summaries = bool(summaries) and bool(model_dir) and dp.rank() == 0
        self._recorders: Dict[str, object] = {}
        self._eval_images = False
        self._step_rate = None
        self._summary_rehearsed = False
        if newest is not None:
            self.restore(newest)

    # ---- checkpoints (checkpoint.py)
    def _run_option(self, name):
        cfg = self.config
        v = cfg.get(name) if isinstance(cfg, dict) else getattr(cfg, name, None)
        return getattr(self.params, name, None) if v is None else v

    def _warm_start(self, ws) -> None:
        """TF warm start: only the ``var/*`` tensors matched by ``vars_to_warm_start`` are
        taken from the file; no moments, no BatchNorm statistics, the step stays 0."""
        if not isinstance(ws, WarmStartSettings):
            ws = WarmStartSettings(os.fspath(ws))
        if dp.world_size() > 1:
            # rank 0 alone reads the file (it may be the only rank that sees it); the broadcast
            # of the parameter arena that follows construction's warm start carries the values.
            # Its verdict is agreed on first, so a bad file raises on every rank.
            err = None
            if dp.rank() == 0:
                try:
                    self._warm_start_local(ws)
                except (C.CheckpointError, OSError) as e:
                    err = f"{type(e).__name__}: {e}"
            err = dp.from_rank0(err)
            if err is not None:
                raise C.CheckpointError(f"warm start failed on rank 0: {err}")
            return
        self._warm_start_local(ws)

    def _warm_start_local(self, ws) -> None:
        path = ws.ckpt_to_initialize_from
        if os.path.isdir(path):
            newest = C.latest_checkpoint(path)
            if newest is None:
                C._refuse_tf(path)
                raise C.CheckpointError(f"{path}: no checkpoint to warm-start from")
            path = newest
        sl = C.StateLayout(self.params, self.engine.layout)
        picked = C.load_warm_start(path, sl, ws.vars_to_warm_start)
        for name, a in picked.items():
            self.engine.P[name].copy_(torch.from_numpy(
                np.ascontiguousarray(self.engine.layout.to_internal(name, a))))

    def restore(self, path) -> None:
        """Load ``path`` into the existing arenas (addresses unchanged, captured steps stay
        valid).  Without a Trainer the optimiser state stays pending until the first TRAIN
        step.  A failed load raises ``CheckpointError`` and leaves the model untouched.

        Under data parallelism every rank calls this and every rank issues the same
        collectives: with a Trainer those of ``Trainer.restore``; without one a MIN all-reduce
        of "I can see the file", a MIN all-reduce of "my load succeeded" (any failure raises on
        every rank, nothing written) and, where not every rank sees the file, two
        ``dp.broadcast_params`` (parameters, BN statistics) from rank 0, whose optimiser state
        follows the same way when the Trainer is made."""
        path = os.fspath(path)
        if self._trainer is not None:
            self._trainer.restore(path, seed_offset=self._seed_offset)
            self._pending = None
        else:
            dev = self.engine.device
            sl = C.StateLayout(self.params, self.engine.layout)
            rank0_only = not dp.all_agree(os.path.exists(path), dev)
            ck = stage = err = None
            if not rank0_only or dp.rank() == 0:
                try:
                    ck = C.load(path, sl)
                    stage = C.stage_verified(ck, sl, dev)
                except C.CheckpointError as e:
                    err = e
            if not dp.all_agree(err is None, dev):
                raise err if err is not None else C.CheckpointError(
                    "restore: another rank could not load the checkpoint; nothing was written")
            if stage is not None:
                self.engine.params.copy_(stage[:sl.n_p])
                self.engine.bn.buf.copy_(stage[sl.o_bn:sl.o_bn + sl.n_bn])
            if rank0_only:
                dp.broadcast_params(self.engine.params)
                dp.broadcast_params(self.engine.bn.buf)
            self._pending = ck if ck is not None else True
            self._pending_rank0_only = rank0_only
        # whatever caches a transform of the weights is rebuilt from the restored ones
        self._eval_decoder = None
        self._host_step = int(dp.from_rank0(
            C.read_meta(path)["global_step"] if dp.rank() == 0 else None))
        self._state_path = path

    def save(self, path=None):
        """Synchronous checkpoint of the training state (``model_dir``'s next file by default)."""
        tr = self._trainer
        if tr is None:
            raise C.CheckpointError("save: no training state yet (run a TRAIN step first)")
        tr.snapshot(self.model_dir, self._run_option("keep_checkpoint_max"), path=path)
        out = tr.wait()
        self._state_path = out
        return out

    def _restore_for(self, checkpoint_path) -> None:
        """EVAL / PREDICT as an Estimator: the named file, else model_dir's newest."""
        if self._trainer is not None:
            self._trainer.wait()
        path = checkpoint_path
        if path is None and self.model_dir:
            path = C.latest_checkpoint(self.model_dir)
        path = None if path is None else os.fspath(path)
        # rank 0's decision holds for every replica (ONE broadcast every rank enters): either
        # all ranks restore, and meet in restore()'s collectives, or none does
        path, do = dp.from_rank0((path, path is not None and path != self._state_path))
        if do:
            self.restore(path)

    @staticmethod
    def learning_rate_decay(init_rate, global_step, step_factor):
        """models/models.py:283-287 (host form; the device form lives in sat_adam_step)."""
        warmup = 4000.0
        step = float(global_step * step_factor + 1)
        return init_rate * warmup ** 0.5 * min(step * warmup ** -1.5, step ** -0.5)

    def _code_batch(self, features, labels):
        """A batch of code targets that is still indices (datasets.CodeBatch): the indices and
        their offsets are uploaded through the stager and ONE launch (sat_codes_batch) writes the
        one-hot ``mel``, ``done``, the two masks and ``target_length`` on the device.  The indices
        are range-checked here on the host, so the kernel's error word is not read back (that
        would make the host wait for the stream every step)."""
        from . import kernels as K
        dev = self.engine.device
        C, r = int(self.params.num_mels), int(self.params.outputs_per_step)
        if r != 1:      # binary_loss_mask is per frame there (datasets/codes/dataset.py:219)
            raise ValueError(f"code batches need outputs_per_step=1, got {r}")
        if int(labels.codes_width) != C:
            raise ValueError(f"code batch of width {labels.codes_width}, hparams.num_mels is {C}")
        idx = np.ascontiguousarray(labels.code_index, dtype=np.int32)
        offsets = np.ascontiguousarray(labels.offsets, dtype=np.int64)
        bad = np.flatnonzero((idx < 0) | (idx >= C))
        if bad.size:
            b = int(np.searchsorted(offsets, bad[0], side="right")) - 1
            raise ValueError(f"code batch: utterance {b}, position {int(bad[0] - offsets[b])}: "
                             f"code index {int(idx[bad[0]])} is outside 0..{C - 1}")
        arrays = {"source": features.source, "source_length": features.source_length,
                  "code_index": idx, "offsets": offsets}
        dtypes = {"source": torch.int64, "source_length": torch.int64,
                  "code_index": torch.int32, "offsets": torch.int64}
        if self.params.use_speaker_embedding:                 # models/models.py:64-70
            if getattr(features, "speaker_id", None) is not None:
                arrays["speaker_id"], dtypes["speaker_id"] = features.speaker_id, torch.int64
            elif self.engine.d.spk_fixed < 0:
                raise ValueError("use_speaker_embedding=True needs features.speaker_id")
        up = self._stager.upload(arrays, dev, dtypes)
        lengths = np.diff(offsets)
        T_pad = -(-int(lengths.max()) // r) * r
        out = K.codes_batch(up.pop("code_index"), up.pop("offsets"), offsets, C=C, T_pad=T_pad,
                            r=r, check=False)
        up.update(mel=out["codes"], mel_mask=out["code_loss_mask"], done=out["done"],
                  done_mask=out["binary_loss_mask"], target_length=out["target_length"])
        return up

    def _batch(self, features, labels):
        if hasattr(labels, "code_index"):
            return self._code_batch(features, labels)
        dev = self.engine.device
        codes = labels.codes if hasattr(labels, "codes") else labels.mel
        cmask = (labels.code_loss_mask if hasattr(labels, "code_loss_mask")
                 else labels.spec_loss_mask)
        arrays = {"source": features.source, "source_length": features.source_length,
                  "mel": codes, "mel_mask": cmask, "done": labels.done,
                  "done_mask": labels.binary_loss_mask, "target_length": labels.target_length}
        if self.params.use_speaker_embedding:                 # models/models.py:64-70
            if getattr(features, "speaker_id", None) is not None:
                arrays["speaker_id"] = features.speaker_id
            elif self.engine.d.spk_fixed < 0:     # speaker_for_synthesis replaces the ids
                raise ValueError("use_speaker_embedding=True needs features.speaker_id")
        i64 = ("source", "source_length", "target_length", "speaker_id")
        dtypes = {k: torch.int64 if k in i64 else torch.float32 for k in arrays}
        return self._stager.upload(arrays, dev, dtypes)

    # ---- summaries (summary.py)
    def _recorder(self, sub: str = ""):
        """The event-file recorder of ``model_dir`` (TRAIN) or ``model_dir/eval``."""
        from . import summary as S
        r = self._recorders.get(sub)
        if r is None:
            logdir = os.path.join(self.model_dir, sub) if sub else self.model_dir
            r = S.SummaryRecorder(S.EventFileWriter(logdir), self.engine.device)
            self._recorders[sub] = r
        return r

    def flush_summaries(self) -> None:
        """Block until every queued summary is in its event file; raise what the writer met."""
        for r in self._recorders.values():
            r.flush()

    def close_summaries(self) -> None:
        recs, self._recorders = self._recorders, {}
        for r in recs.values():
            r.close()

    def _image_groups(self, batch, features, labels, al1, al2, mel, mel_target, enc_probs=(),
                      dec_probs=()):
        """The reference's MetricsSaver plots for the first min(B, 3) utterances as
        summary.ImageGroup lists.  Every stride and canvas size comes from the plotted tensor's
        own shape (a captured step may have padded T' beyond the caller's batch,
        StepGraphCache._pad_t); the crops come from the batch's lengths.  ``al1`` / ``al2`` =
        (tensor, offset of step 0 of utterance 0, utterance stride, step stride, steps) of an
        alignment history whose memory axis is contiguous; ``mel`` / ``mel_target`` [B, T, M];
        ``enc_probs`` / ``dec_probs`` [B, H, L, L] softmax probabilities per hop."""
        from .summary import ImageGroup
        r = self.params.outputs_per_step
        B, N = batch["source"].shape
        k = min(B, 3)
        T_all = min(mel.shape[1], mel_target.shape[1])
        src_len = batch["source_length"][:k].to(torch.int32)
        tgt_len = batch["target_length"][:k].to(torch.int32).clamp(max=T_all)
        stp_len = ((tgt_len + (r - 1)) // r).clamp(max=min(al1[4], al2[4]))
        dev = src_len.device

        def host(x, f=lambda v: v):
            # the host's own copy of the lengths, when it was given one: the kernels' entries
            # then check the crops against the canvas before launching
            return [f(int(v)) for v in np.asarray(x)[:k]] if isinstance(x, np.ndarray) else None
        h_src = host(getattr(features, "source_length", None))
        h_tgt = host(getattr(labels, "target_length", None), lambda v: min(v, T_all))
        h_stp = host(getattr(labels, "target_length", None),
                     lambda v: min((v + r - 1) // r, al1[4], al2[4]))
        out = []
        for name, (a, off, utt, col, steps) in (("alignment1", al1), ("alignment2", al2)):
            out.append(ImageGroup([f"{name}/{i}" for i in range(k)], a, off, utt, src_len,
                                  stp_len, col, N, steps, h_src, h_stp))
        for what, probs, ln, h_ln in (("encoder_self_attention", enc_probs, src_len, h_src),
                                      ("decoder_self_attention", dec_probs, stp_len, h_stp)):
            for hop, p in enumerate(probs):
                _, H, L, _ = p.shape
                for h in range(H):
                    out.append(ImageGroup([f"{what}{hop}_head{h}/{i}" for i in range(k)], p,
                                          h * L * L, H * L * L, ln, ln, L, L, L, h_ln, h_ln))
        for name, x in (("mel_predicted", mel), ("mel_target", mel_target)):
            _, T, M = x.shape
            bins = torch.full((k,), M, dtype=torch.int32, device=dev)
            out.append(ImageGroup([f"{name}/{i}" for i in range(k)], x, 0, T * M, bins, tgt_len,
                                  M, M, T, [M] * k, h_tgt))
        return out

    def _reserve_train_summaries(self, batch) -> None:
        """Size the recorder's staging slots for this batch shape's plots.  Called on every
        TRAIN step (integer arithmetic); allocates only when a larger shape is first seen --
        the step that also allocates that shape's buffers and captures its graph."""
        from .summary import ImageGroup
        hp = self.params
        B, N = batch["source"].shape
        T, M = batch["mel"].shape[1], batch["mel"].shape[2]
        r = hp.outputs_per_step
        q = self.graph_t_quantum if self.graph_cache > 0 else 0
        Tp = -(-(T // r) // q) * q if q > 0 else T // r
        k = min(B, 3)
        need = 256 + 2 * ImageGroup.nbytes(k, N, Tp + 1) + 2 * ImageGroup.nbytes(k, M, Tp * r)
        self._recorder().reserve(need)

    def _train_summaries(self, batch, features, labels) -> None:
        """After a TRAIN step (eager or a replay; never inside a capture): queue the step's
        scalars and, when due, its images, on the training stream (summary.SummaryRecorder)."""
        from . import summary as S
        step = self._host_step
        self._reserve_train_summaries(batch)
        if self._step_rate is None:
            self._step_rate = S.StepRate(self._run_option("log_step_count_steps"))
        rate = self._step_rate.tick(step)
        every = int(self._run_option("save_summary_steps") or 0)
        img_every = int(self._run_option("alignment_save_steps") or 0)
        scalars = every > 0 and step % every == 0
        images = (img_every > 0 and step % img_every == 0
                  and bool(self._run_option("save_training_time_metrics")))
        rec = self._graphs.last_record
        # the first TRAIN step rehearses a full summary (SummaryRecorder.record, step=None)
        rehearse = not self._summary_rehearsed and rec is not None and not (scalars and images)
        if rehearse:
            self._summary_rehearsed = True
            want = (scalars, images)
            scalars = True
            images = bool(self._run_option("save_training_time_metrics"))
            self._record_train(None, rec, batch, features, labels, scalars, images, None)
            scalars, images = want
        if not (scalars or images) or rec is None:
            return
        self._record_train(step, rec, batch, features, labels, scalars, images, rate)

    def _record_train(self, step, rec, batch, features, labels, scalars, images, rate) -> None:
        out, sv = rec
        floats, names, groups, extra = [], [], [], {}
        if scalars:
            # loss[0:3] = {0.1 L1 + BCE, L1, BCE}; Trainer.scalars = {norm, clip scale, lr, lr_t}
            code = 0.1 * out["l1"]
            # (TRAIN is teacher-forced: add_training_stats writes each loss under both tags)
            floats = [out["loss"], code, code, out["bce"], out["bce"], self._trainer.scalars]
            names = ["loss_with_teacher", "code_loss", "code_loss_with_teacher", "done_loss",
                     "done_loss_with_teacher", "global_norm", None, "learning_rate", None]
            extra = {"l2_regularization_loss": 0.0}
            if rate is not None:
                extra["global_step/sec"] = rate
        if images:
            # the step's own tensors: under graph_t_quantum their T' is the padded one
            dec = sv["dec"]
            Tp, B, N = dec.S2.shape
            if tuple(dec.AL1.shape) != (Tp + 1, B, N) or B != batch["source"].shape[0]:
                raise RuntimeError("alignment histories are not [T' + 1, B, N] / [T', B, N]")
            # (no encoder self-attention plot in TRAIN: the fused attention keeps no
            # probabilities; EVAL's decode materialises them and plots them)
            groups = self._image_groups(batch, features, labels, (dec.AL1, B * N, N, B * N, Tp),
                                        (dec.S2, 0, N, B * N, Tp), sv["mel"], sv["batch"]["mel"])
        self._recorder().record(step, floats, names, groups, extra)

    def _eval_summaries(self, batch, features, labels, spec) -> None:
        """EVAL's plots (MetricsSaver with alignment_save_steps = 1, models/models.py:238-247)
        of an evaluated batch, at the restored global step, into ``model_dir/eval``."""
        mt = spec.eval_metric_ops
        B, N = batch["source"].shape
        als = []
        for key in ("alignment1", "alignment2"):
            a = mt[key]                                          # [B, N, T']
            if tuple(a.shape[:2]) != (B, N):
                raise RuntimeError(f"{key} is not [B, N, T']")
            Tp = a.shape[2]
            als.append((a.transpose(1, 2).contiguous(), 0, Tp * N, N, Tp))
        probs = {k: [p.contiguous() for p in mt[k] if p is not None]
                 for k in ("encoder_self_alignments", "decoder_self_alignments")}
        groups = self._image_groups(batch, features, labels, als[0], als[1],
                                    spec.predictions["mel"].contiguous(), batch["mel"],
                                    enc_probs=probs["encoder_self_alignments"],
                                    dec_probs=probs["decoder_self_alignments"])
        self._recorder("eval").record(self._host_step, groups=groups)

    def _get_trainer(self, batch) -> Trainer:
        """ONE trainer (one optimiser state) for every batch shape: its mask views are re-pointed
        per shape inside one arena (Trainer.reshape), so memory stays flat over a stream of
        differently padded batches."""
        B, N = batch["source"].shape
        Tp = batch["mel"].shape[1] // self.params.outputs_per_step
        if self._trainer is None:
            self._trainer = Trainer(self.engine, B, N, Tp, seed=self._seed)
            self._trainer.keep_saved = self.summaries
            if self._pending is not None:
                # optimiser state, step, seed and status of the restore made before any TRAIN
                ck, self._pending = self._pending, None
                self._trainer.restore(ck if ck is not True else None,
                                      seed_offset=self._seed_offset,
                                      rank0_only=self._pending_rank0_only)
        return self._trainer

    def _infer_seed(self) -> Optional[torch.Tensor]:
        """The inference seed word (made on first use); None with the switch off, where no
        decoder reads a seed and nothing is allocated."""
        if not getattr(self.params, "apply_dropout_on_inference", False):
            return None
        if self._infer_seed_dev is None:
            self._infer_seed_dev = torch.tensor([self._seed], dtype=torch.int64,
                                                device=self.engine.device)
        return self._infer_seed_dev

    def _teacher_masks(self, batch):
        """The masks of a teacher-forced pass outside training (models/models.py:134, :223 hand
        ``apply_dropout_on_inference`` to the decoder): None with the switch off, else the
        decoder prenet masks ``dec/prenet{l}`` [T', B, P_l] of the dropping layers, drawn from
        the inference seed (which advances); everything else keeps eval semantics."""
        if not getattr(self.params, "apply_dropout_on_inference", False):
            return None
        from .inference import advance_seed, draw_prenet_masks
        B = batch["source"].shape[0]
        Tp = batch["mel"].shape[1] // self.params.outputs_per_step
        seed = self._infer_seed()
        masks = draw_prenet_masks(self.engine.d, Tp, B,
                                  1.0 - float(self.params.decoder_prenet_drop_rate), seed)
        advance_seed(seed)
        return masks

    def _predict(self, features) -> EstimatorSpec:
        """PREDICT (models/models.py:84-97, 252-277): free-running decode (inference.py) and
        the reference's predictions dict.  ``codes`` follows the fork's one-hot of the argmax
        over the feature bins of each frame (:99-100); ``mel`` is the raw decoder output
        (code_output_raw) the one-hot is taken from."""
        from .inference import FreeRunningDecoder
        dev = self.engine.device
        batch = {"source": _to_device(features.source, dev, torch.int64),
                 "source_length": _to_device(features.source_length, dev, torch.int64)}
        if self.params.use_speaker_embedding:
            if getattr(features, "speaker_id", None) is not None:
                batch["speaker_id"] = _to_device(features.speaker_id, dev, torch.int64)
            elif self.engine.d.spk_fixed < 0:     # speaker_for_synthesis replaces the ids
                raise ValueError("use_speaker_embedding=True needs features.speaker_id")
        out = FreeRunningDecoder(self.engine, max_iters=self.params.max_iters,
                                 seed=self._infer_seed()).run(batch)
        mel = out["mel"]
        codes = torch.zeros_like(mel)
        codes.scatter_(2, mel.argmax(dim=2, keepdim=True), 1.0)       # tf.one_hot(argmax)
        preds = {"id": features.id, "key": features.key, "codes": codes, "mel": mel,
                 "stop_token": out["stop"], "alignment": out["alignment1"],
                 "alignment2": out["alignment2"], "source": features.source,
                 "text": getattr(features, "text", None),
                 # what the plot and the prediction record of a synthesis crop by and compare
                 # with (predict_mel.py:50-53); absent where the features carry no target
                 "source_length": features.source_length,
                 "ground_truth_mel": getattr(features, "mel", None),
                 "ground_truth_mel_length": getattr(features, "target_length", None)}
        # decoder self-attention alignments (per hop, per head, transposed as :108-109), then
        # the encoder's (alignment5..8)
        dec = [a[:, h].transpose(1, 2) for a in out["decoder_self_alignments"]
               for h in range(a.shape[1])]
        for i, a in enumerate(dec[:2]):
            preds[f"alignment{3 + i}"] = a
        enc = [a[:, h].transpose(1, 2) for a in out["encoder_self_alignments"]
               for h in range(a.shape[1])]
        for i, a in enumerate(enc[:4]):
            preds[f"alignment{5 + i}"] = a
        preds = {k: v for k, v in preds.items() if v is not None}
        return EstimatorSpec(ModeKeys.PREDICT, loss=None, train_op=None, predictions=preds,
                             eval_metric_ops=None)

    def forced_alignment_pass(self, batch) -> Dict[str, object]:
        """``use_forced_alignment_mode`` (models/models.py:84-97, 118-148): a teacher-forced
        validation pass (eval semantics; equal to the training-branch decoder by
        modules/transformer_test.py:44-90) yields the alignment histories, then a second pass
        decodes with ``force_alignment_dual_source_attention_factory`` mechanisms
        (TeacherForcing*Attention replaying those alignments) under
        ``OneHotValidationHelper(teacher_forcing=False)`` (softmax feedback, exactly T' steps).
        Returns the second pass's outputs (the ones the reference's loss and predictions use)
        with its alignment histories [B, N, T'] and the teacher-forced first pass's."""
        from .attentions import force_alignment_dual_source_attention_factory
        from .inference import FreeRunningDecoder
        hp = self.params
        kinds = (hp.forced_alignment_attention, hp.forced_alignment_attention2)
        for k in kinds:
            if k not in ("teacher_forcing_forward", "teacher_forcing_additive"):
                raise ValueError(f"forced_alignment_attention must be a teacher_forcing kind: {k}")
        force_alignment_dual_source_attention_factory(hp)          # option checks
        with torch.no_grad():
            first, _ = self.engine.forward(batch, self._teacher_masks(batch), training=False,
                                           need_grad=False)
            a1 = first["alignment1"].permute(1, 0, 2).contiguous()    # [B, T', N]
            a2 = first["alignment2"].permute(1, 0, 2).contiguous()
            dec = FreeRunningDecoder(self.engine, forced_alignments=(a1, a2), feed="softmax",
                                     seed=self._infer_seed())
            out = dec.run(batch)
        out["teacher_alignment1"] = a1.transpose(1, 2)
        out["teacher_alignment2"] = a2.transpose(1, 2)
        return out

    def _loss_of(self, mel, stop, batch):
        """0.1 * codes_loss + binary_loss (models/models.py:159-173) of a decode's outputs."""
        from . import kernels as K
        loss = torch.zeros(8, device=mel.device)
        K.loss_fwd_bwd(mel.contiguous(), batch["mel"], batch["mel_mask"], stop.contiguous(),
                       batch["done"], batch["done_mask"], loss)
        return loss

    def validation_pass(self, batch) -> Dict[str, object]:
        """EVAL's own decode (models/models.py:86-97 with is_validation=True,
        teacher_forcing=False): OneHotValidationHelper (modules/helpers.py:61-108) -- exactly
        T' = T/r steps with real attention, step t+1 fed the per-frame softmax of step t's
        output."""
        from .inference import FreeRunningDecoder
        if self._eval_decoder is None:
            self._eval_decoder = FreeRunningDecoder(self.engine, helper="validation",
                                                    feed="softmax", seed=self._infer_seed())
        return self._eval_decoder.run(batch)

    def _eval(self, batch) -> EstimatorSpec:
        """EVAL (models/models.py:84-97, 151-173, 208-235, 305-320):
        * ``loss`` / ``code_loss`` / ``done_loss`` of the validation decode (softmax feedback,
          T' steps; under ``use_forced_alignment_mode`` the forced second pass instead);
        * ``loss_with_teacher`` / ``code_loss_with_teacher`` / ``done_loss_with_teacher`` of the
          teacher-forced pass (validation with teacher forcing, equal to the training branch
          in eval mode by modules/transformer_test.py:44-90)."""
        hp = self.params
        with torch.no_grad():
            if getattr(hp, "use_forced_alignment_mode", False):
                out = self.forced_alignment_pass(batch)
            else:
                out = self.validation_pass(batch)
            l = self._loss_of(out["mel"], out["stop"], batch)
            teach, _ = self.engine.forward(batch, self._teacher_masks(batch), training=False,
                                           need_grad=False)
        code_loss, done_loss = 0.1 * l[1:2], l[2:3]
        loss = code_loss + done_loss                                  # + regularization (0)
        metrics = {"code_loss": code_loss, "done_loss": done_loss,
                   "loss_with_teacher": teach["loss"],
                   "code_loss_with_teacher": 0.1 * teach["l1"],
                   "done_loss_with_teacher": teach["bce"],
                   "alignment1": out["alignment1"], "alignment2": out["alignment2"],
                   "l2_regularization_loss": torch.zeros_like(done_loss),
                   "decoder_self_alignments": out.get("decoder_self_alignments") or [],
                   "encoder_self_alignments": out.get("encoder_self_alignments") or []}
        return EstimatorSpec(ModeKeys.EVAL, loss=loss, train_op=None,
                             predictions={"mel": out["mel"], "stop_token": out["stop"]},
                             eval_metric_ops=metrics)

    def model_fn(self, features, labels, mode, params=None) -> EstimatorSpec:
        if mode == ModeKeys.PREDICT:
            return self._predict(features)
        batch = self._batch(features, labels)
        if mode == ModeKeys.TRAIN:
            # one captured step per padded batch shape, replayed when the shape comes back
            # (train.StepGraphCache; eager on a first sighting or with graph_cache=0)
            tr = self._get_trainer(batch)
            if self._graphs is None:
                self._graphs = StepGraphCache(tr, self.graph_cache, self.graph_t_quantum)
            out = self._graphs.step(batch)
            self._host_step += 1
            self._state_path = None
            if self.summaries:
                self._train_summaries(batch, features, labels)
            return EstimatorSpec(mode, loss=out["loss"], train_op=tr.global_step,
                                 predictions=None, eval_metric_ops=None)
        if mode == ModeKeys.EVAL:
            spec = self._eval(batch)
            if self.summaries and self._eval_images:
                self._eval_images = False
                self._eval_summaries(batch, features, labels, spec)
            return spec
        raise ValueError(f"Unknown mode: {mode}")

    # ---- tf.estimator.Estimator-like drivers
    def predict(self, input_fn, checkpoint_path=None):
        """``checkpoint_path`` (predict_mel.py:67-68) or model_dir's newest file is restored
        before the first batch."""
        self._restore_for(checkpoint_path)
        for features, _ in input_fn():
            yield self.model_fn(features, None, ModeKeys.PREDICT, self.params).predictions

    def train(self, input_fn, steps: int):
        """With a ``model_dir``: a snapshot whenever the step count reaches a multiple of
        ``save_checkpoints_steps`` (queued, the loop does not wait for it) and a last one at the
        end, which is waited for; ``keep_checkpoint_max`` files are kept."""
        loss = None
        it = iter(input_fn())
        every = int(self._run_option("save_checkpoints_steps") or 0) if self.model_dir else 0
        keep = self._run_option("keep_checkpoint_max")
        saved_at = None
        for _ in range(steps):
            features, labels = next(it)
            loss = self.model_fn(features, labels, ModeKeys.TRAIN, self.params).loss
            if every > 0 and self._host_step % every == 0:
                self._trainer.snapshot(self.model_dir, keep)
                saved_at = self._host_step
        if self.model_dir and self._trainer is not None:
            self._trainer.wait()
            if saved_at != self._host_step and steps > 0:
                self._trainer.snapshot(self.model_dir, keep)
            self._state_path = self._trainer.wait()      # rank 0: the file; others: None
        if self.summaries:
            self.flush_summaries()
        return loss

    def evaluate(self, input_fn, steps: int = 1, checkpoint_path=None):
        """``loss`` and the streaming means of the reference's validation metrics
        (get_validation_metrics, models/models.py:304-320) over ``steps`` batches, with the
        ``global_step`` of the evaluated state.  With ``summaries``: the metrics, and the plots
        of the first batch, go to ``model_dir/eval`` at that step."""
        from .summary import EVAL_METRICS
        self._restore_for(checkpoint_path)
        tot = 0.0
        sums = dict.fromkeys(EVAL_METRICS, 0.0)
        it = iter(input_fn())
        self._eval_images = True                   # the first batch's plots (summaries only)
        for _ in range(steps):
            features, labels = next(it)
            spec = self.model_fn(features, labels, ModeKeys.EVAL, self.params)
            tot += float(spec.loss.item())
            for k in EVAL_METRICS:
                sums[k] += float(spec.eval_metric_ops[k].item())
        out = {"loss": tot / steps}
        out.update((k, v / steps) for k, v in sums.items())
        if self.summaries:
            w = self._recorder("eval")
            w.writer.add_scalars(self._host_step, out)
            w.flush()
        out["global_step"] = self._host_step
        return out


def tacotron_model_factory(hparams, model_dir, run_config, warm_start_from=None, **kw):
    if hparams.tacotron_model == "DualSourceSelfAttentionTacotronModel":
        return DualSourceSelfAttentionTacotronModel(hparams, model_dir, config=run_config,
                                                    warm_start_from=warm_start_from, **kw)
    raise ValueError(f"Unknown Tacotron model: {hparams.tacotron_model}")


def synthetic_input_fn(params, batch_size: int, N: int = 200, T: int = 1000, shape="max",
                       seed: int = 0):
    """An input_fn over seeded synthetic batches with the dataset contract of SURVEY.md 8(d)."""
    from . import data

    def input_fn():
        step = 0
        while True:
            b = data.synthetic_batch(params, batch_size, N=N, T=T, seed=seed + step, shape=shape)
            step += 1
            ids = np.arange(batch_size)
            if "speaker_id" in b:
                yield (SourceData(ids, ids, b["source"], b["source_length"], b["speaker_id"],
                                  None, None, None),
                       MelData(ids, ids, b["mel"], params.num_mels, b["target_length"],
                               b["done"], b["mel_mask"], b["done_mask"]))
                continue
            yield (PreprocessedSourceData(ids, ids, b["source"], b["source_length"], None),
                   PreprocessedTargetData(ids, ids, b["mel"], b["target_length"], b["done"],
                                          b["mel_mask"], b["done_mask"]))
    return input_fn


from .summary import train_and_evaluate  # noqa: E402,F401  (tf.estimator.train_and_evaluate)
