"""Training summaries: TensorBoard event files of scalars and alignment images, without
TensorFlow.

What the reference writes through ``tf.summary`` and its ``MetricsSaver`` hook
(models/models.py:185-199, 238-247, 289-320): the loss scalars and the learning rate every
``save_summary_steps`` steps, the alignment / self-attention / mel plots of the first utterances
every ``alignment_save_steps`` steps, the EVAL metrics under ``model_dir/eval``.

* ``encode_png``: 8-bit grayscale PNG with ``zlib`` + ``struct`` only.
* ``EventFileWriter``: ``events.out.tfevents.<unix seconds>.<hostname>`` -- TFRecord-framed
  (``tfrecord.frame_record``) ``Event`` protobufs (``tfrecord._varint`` / ``_ld``), the first
  carrying ``file_version = "brain.Event:2"``.  ONE writer thread appends; callers only queue.
* ``SummaryRecorder``: the device half.  After a step (eager or a graph replay, never inside a
  capture) it queues, on the training stream, the copies of the step's scalars and the image
  kernels (csrc/summary.hip) into a staging slot; a side stream copies the slot to pinned
  memory behind an event, followed by a sequence word the writer thread polls (no device API
  call on that thread, as checkpoint.Snapshotter).  The slots and their pinned mirrors are
  allocated when the recorder is made and when a larger batch shape is first seen, never in a
  step that writes; a step that writes issues device work only (no host-to-device copy).
"""

from __future__ import annotations

import os
import queue
import socket
import struct
import threading
import time
import zlib
from collections import deque
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import tfrecord

FILE_VERSION = "brain.Event:2"
TRAIN_SCALAR_TAGS = ("loss_with_teacher", "code_loss", "code_loss_with_teacher", "done_loss",
                     "done_loss_with_teacher", "learning_rate", "l2_regularization_loss",
                     "global_norm")
EVAL_METRICS = ("code_loss", "done_loss", "loss_with_teacher", "code_loss_with_teacher",
                "done_loss_with_teacher", "l2_regularization_loss")


class SummaryError(RuntimeError):
    """A summary could not be written (raised from the call after the one that queued it)."""


# ---------------------------------------------------------------- PNG
def _chunk(kind: bytes, body: bytes) -> bytes:
    return (struct.pack(">I", len(body)) + kind + body
            + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF))


def encode_png(image: np.ndarray, level: int = 6) -> bytes:
    """uint8 [height, width] -> an 8-bit grayscale PNG (filter 0 on every line)."""
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"encode_png: a non-empty uint8 [H, W] array, got {a.dtype} {a.shape}")
    h, w = a.shape
    raw = np.zeros((h, w + 1), np.uint8)
    raw[:, 1:] = a
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b""))


# ---------------------------------------------------------------- Event protobufs
_v, _ld = tfrecord._varint, tfrecord._ld


def scalar_value(tag: str, value: float) -> bytes:
    """Summary.Value{tag = 1, simple_value = 2 (float)}."""
    return _ld(1, tag.encode("utf-8")) + _v(2 << 3 | 5) + struct.pack("<f", value)


def image_value(tag: str, image: np.ndarray) -> bytes:
    """Summary.Value{tag = 1, image = 4: Image{height = 1, width = 2, colorspace = 3 (1:
    grayscale), encoded_image_string = 4 (PNG)}}."""
    h, w = image.shape
    img = (_v(1 << 3) + _v(h) + _v(2 << 3) + _v(w) + _v(3 << 3) + _v(1)
           + _ld(4, encode_png(image)))
    return _ld(1, tag.encode("utf-8")) + _ld(4, img)


def event(wall_time: float, step: int = 0, values: Sequence[bytes] = (),
          file_version: Optional[str] = None) -> bytes:
    """Event{wall_time = 1 (double), step = 2, file_version = 3 | summary = 5:
    Summary{value = 1 (repeated)}}."""
    out = _v(1 << 3 | 1) + struct.pack("<d", wall_time)
    if step:
        out += _v(2 << 3) + _v(step)
    if file_version is not None:
        out += _ld(3, file_version.encode("utf-8"))
    if values:
        out += _ld(5, b"".join(_ld(1, v) for v in values))
    return out


# ---------------------------------------------------------------- the writer thread
class EventFileWriter:
    """Appends events to ``logdir/events.out.tfevents.<unix seconds>.<hostname>``.

    Every ``add_*`` only queues; ONE thread creates the directory and the file when the first
    event arrives, frames and appends.  ``flush()`` / ``close()`` drain the queue.  What the
    thread could not do (an unwritable directory, a device copy that never arrived) is raised
    as ``SummaryError`` from the next call; events queued behind a failure are dropped, and a
    file is created only once its first record can be written whole."""

    def __init__(self, logdir: str, clock: Callable[[], float] = time.time):
        self.logdir = os.fspath(logdir)
        self.clock = clock
        self.path: Optional[str] = None
        self._q: "queue.Queue" = queue.Queue()
        self._err: Optional[BaseException] = None
        self._file = None
        self._closed = False
        self._thread = threading.Thread(target=self._run, name="sat-summary", daemon=True)
        self._thread.start()

    # ---- writer thread
    def _open(self):
        os.makedirs(self.logdir, exist_ok=True)
        name = f"events.out.tfevents.{int(self.clock())}.{socket.gethostname()}"
        path = os.path.join(self.logdir, name)
        f = open(path, "ab")
        try:
            f.write(tfrecord.frame_record(event(self.clock(), file_version=FILE_VERSION)))
            f.flush()
        except BaseException:
            f.close()
            os.unlink(path)
            raise
        self._file, self.path = f, path

    def _run(self):
        while True:
            job = self._q.get()
            try:
                if job is None:
                    return
                step, make, drop = job
                if self._err is not None:
                    if drop is not None:
                        drop()
                    continue                      # dropped: the failure is reported first
                wall, values = make()
                if not values:
                    continue
                if self._file is None:
                    self._open()
                self._file.write(tfrecord.frame_record(event(wall, step, values)))
                self._file.flush()
            except BaseException as e:            # noqa: BLE001 -- handed to the caller
                self._err = e
            finally:
                self._q.task_done()

    # ---- callers
    def _raise_pending(self):
        e, self._err = self._err, None
        if e is not None:
            raise SummaryError(f"summary writer ({self.logdir}): {type(e).__name__}: {e}") from e

    def add_deferred(self, step: int, make: Callable[[], Tuple[float, List[bytes]]],
                     drop: Optional[Callable[[], None]] = None) -> None:
        """Queue ``make`` (run on the writer thread) -> (wall_time, [Summary.Value bytes]);
        ``drop`` runs instead when the event is dropped behind a failure."""
        if self._closed:
            raise SummaryError("summary writer is closed")
        self._raise_pending()
        self._q.put((int(step), make, drop))

    def add_scalars(self, step: int, scalars: Dict[str, float]) -> None:
        wall = self.clock()
        vals = [scalar_value(k, float(v)) for k, v in scalars.items()]
        self.add_deferred(step, lambda: (wall, vals))

    def flush(self) -> None:
        self._q.join()
        self._raise_pending()

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        self._q.join()
        self._q.put(None)
        self._thread.join()
        if self._file is not None:
            self._file.close()
            self._file = None
        self._raise_pending()


# ---------------------------------------------------------------- the device half
class _Slot:
    """One staging arena on the device, its pinned mirror and the sequence word of its copy."""

    def __init__(self, device, nbytes: int):
        import torch
        self.device = device
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.host = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True)
        self.seq = torch.zeros(2, dtype=torch.int32, device=device)
        self.seq_host = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        self.seq_np = self.seq_host.numpy()
        self.free = threading.Event()
        self.free.set()
        self.used = 0

    def grow(self, nbytes: int) -> None:
        """Replace the arena by a larger one (the slot must be free)."""
        import torch
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.host = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True)

    def take(self, nbytes: int, dtype):
        """The next ``nbytes`` of the arena (16-byte aligned) as a ``dtype`` view -> (view, off)."""
        off = (self.used + 15) // 16 * 16
        self.used = off + nbytes
        assert self.used <= self.dev.numel()
        return self.dev[off:off + nbytes].view(dtype), off


class ImageGroup:
    """``k`` images of one source tensor: element (r, c) of image i at ``src.flatten()[base0 +
    i * base_stride + c * col_stride + r]``, crop ``rows[i] x cols[i]`` (device int32), canvas
    Rmax x Cmax; ``tags[i]`` names image i (``k = len(tags)``)."""

    def __init__(self, tags, src, base0, base_stride, rows, cols, col_stride, Rmax, Cmax,
                 rows_host=None, cols_host=None):
        self.tags, self.src = list(tags), src
        self.base0, self.base_stride = int(base0), int(base_stride)
        self.rows, self.cols, self.col_stride = rows, cols, int(col_stride)
        self.Rmax, self.Cmax = int(Rmax), int(Cmax)
        self.rows_host, self.cols_host = rows_host, cols_host

    @staticmethod
    def nbytes(k: int, Rmax: int, Cmax: int) -> int:
        """Staging bytes of a group: min / max, counts, the two crop arrays, the canvases."""
        return 5 * 16 + 20 * k + k * Rmax * Cmax


class SummaryRecorder:
    """Device -> event file (see the module docstring).

    ``record(step, floats, names, groups, extra)``: ``floats`` are small float32 device tensors
    whose elements become the scalars ``names`` (None skips an element); ``groups`` the images;
    ``extra`` host-side scalars added as they are.  A ring of ``depth`` slots, allocated here
    (pinned allocation is slow and may wait for the device: it belongs to construction, not to
    a step): a slot is reused once the writer thread has copied its pinned bytes out.

    What the training thread may wait for: the writer, when it is ``depth`` summaries behind;
    and ``reserve()`` -- called where a larger batch shape is first seen, a step that allocates
    and captures anyway -- which waits for the slots to be free before it replaces them.
    ``record()`` itself grows a slot only if ``reserve()`` was not told of the shape."""

    def __init__(self, writer: EventFileWriter, device, depth: int = 3, nbytes: int = 1 << 16):
        import torch
        self.writer = writer
        self.device = torch.device(device)
        self.capacity = int(nbytes)
        self.slots = [_Slot(self.device, self.capacity) for _ in range(depth)]
        self.i = 0
        self.count = 0
        self.side = torch.cuda.Stream(device=self.device)
        self._ramps: Dict[int, object] = {}
        self.timeout_s = 120.0
        self._cancel = threading.Event()

    def reserve(self, nbytes: int) -> None:
        """Make every slot hold ``nbytes``.  Replaces the arenas (a pinned allocation each), so
        it waits for summaries still in flight: call it where a new shape is first seen."""
        if nbytes <= self.capacity:
            return
        self.capacity = int(nbytes)
        for slot in self.slots:
            slot.free.wait()
            slot.grow(self.capacity)

    def _base(self, g: ImageGroup, k: int):
        """base[i] = base0 + i * base_stride, made on the device from a cached 0..k-1 ramp (no
        host-to-device copy, which from pageable memory would drain the stream)."""
        import torch
        ramp = self._ramps.get(k)
        if ramp is None:
            ramp = torch.arange(k, dtype=torch.int64, device=self.device)
            self._ramps[k] = ramp
        return ramp * g.base_stride + g.base0

    def record(self, step: Optional[int], floats=(), names: Sequence[Optional[str]] = (),
               groups: Sequence[ImageGroup] = (), extra: Optional[Dict[str, float]] = None):
        """``step=None`` is a rehearsal: the same device work into a slot, nothing queued for
        the file.  The first use of each kernel and tensor operation loads its code object
        (tens of milliseconds on the host); the model rehearses on its first TRAIN step, which
        allocates and captures anyway, so that no later step pays for it."""
        import torch
        from . import kernels as K
        self.writer._raise_pending()
        nf = sum(int(f.numel()) for f in floats)
        assert nf == len(names)
        need = 32 + 4 * nf + sum(ImageGroup.nbytes(len(g.tags), g.Rmax, g.Cmax) for g in groups)
        self.reserve(need)
        slot = self.slots[self.i]
        self.i = (self.i + 1) % len(self.slots)
        slot.free.wait()
        slot.free.clear()
        try:
            slot.used = 0
            plan = []
            if nf:
                fv, off = slot.take(4 * nf, torch.float32)
                o = 0
                for f in floats:
                    fv[o:o + f.numel()].copy_(f.reshape(-1))
                    o += f.numel()
                plan.append(("floats", off, nf, list(names)))
            for g in groups:
                k = len(g.tags)
                if k == 0 or g.Rmax < 1 or g.Cmax < 1:
                    continue
                base = self._base(g, k)
                mm, _ = slot.take(8 * k, torch.float32)
                bad, o_bad = slot.take(4 * k, torch.int32)
                rows, o_rows = slot.take(4 * k, torch.int32)
                cols, o_cols = slot.take(4 * k, torch.int32)
                canvas, o_img = slot.take(k * g.Rmax * g.Cmax, torch.uint8)
                rows.copy_(g.rows)
                cols.copy_(g.cols)
                K.image_minmax(g.src, base, rows, cols, g.col_stride, g.Rmax, g.Cmax, mm, bad,
                               g.rows_host, g.cols_host)
                K.image_render(g.src, base, rows, cols, g.col_stride, mm,
                               canvas.view(k, g.Rmax, g.Cmax), g.rows_host, g.cols_host)
                plan.append(("images", (o_bad, o_rows, o_cols, o_img), (k, g.Rmax, g.Cmax),
                             g.tags))
            self.count += 1
            count = self.count
            slot.seq.fill_(count)
            ready = torch.cuda.Event()
            ready.record()
            used, host = slot.used, slot.host
            with torch.cuda.stream(self.side):
                self.side.wait_event(ready)
                host[:used].copy_(slot.dev[:used], non_blocking=True)
                slot.seq_host.copy_(slot.seq, non_blocking=True)  # last: the writer's signal
            if step is None:
                slot.free.set()      # later users of the slot are stream-ordered behind this
                return
            wall = self.writer.clock()
            extra = dict(extra or {})
            self.writer.add_deferred(
                step, lambda: self._make(slot, host, used, count, plan, wall, extra),
                drop=slot.free.set)
        except BaseException:
            slot.free.set()          # a refused launch or a closed writer must not strand it
            raise

    def _make(self, slot: _Slot, host, used: int, count: int, plan, wall: float, extra):
        """Writer thread: wait for the slot's copy, take its bytes, free it, encode."""
        try:
            t0 = time.monotonic()
            while int(slot.seq_np[0]) != count:
                if (time.monotonic() - t0 > self.timeout_s or self._cancel.is_set()
                        or not threading.main_thread().is_alive()):
                    raise SummaryError("the device-to-host copy of a summary did not arrive")
                time.sleep(0.0005)
            raw = host.numpy()[:used].copy()
        finally:
            slot.free.set()
        values = []
        for kind, off, n, names in plan:
            if kind == "floats":
                v = raw[off:off + 4 * n].view("<f4")
                values += [_ld(1, nm.encode("utf-8")) + _v(2 << 3 | 5) + v[j:j + 1].tobytes()
                           for j, nm in enumerate(names) if nm is not None]
                continue
            (o_bad, o_rows, o_cols, o_img), (k, R, C) = off, n
            rows = raw[o_rows:o_rows + 4 * k].view("<i4")
            cols = raw[o_cols:o_cols + 4 * k].view("<i4")
            canvas = raw[o_img:o_img + k * R * C].reshape(k, R, C)
            for j, tag in enumerate(names):
                r, c = min(max(int(rows[j]), 0), R), min(max(int(cols[j]), 0), C)
                if r and c:
                    values.append(image_value(tag, canvas[j, :r, :c]))
        values += [scalar_value(k, v) for k, v in extra.items()]
        return wall, values

    def flush(self) -> None:
        self.writer.flush()

    def close(self) -> None:
        self._cancel.set()
        self.writer.close()


class StepRate:
    """``global_step/sec`` as the Estimator's StepCounterHook: steps over host seconds across
    the last ``every`` steps."""

    def __init__(self, every: int, clock: Callable[[], float] = time.monotonic):
        self.every = max(int(every or 1), 1)
        self.clock = clock
        self.marks: deque = deque(maxlen=self.every + 1)

    def tick(self, step: int) -> Optional[float]:
        self.marks.append((int(step), self.clock()))
        if len(self.marks) <= self.every:
            return None
        (s0, t0), (s1, t1) = self.marks[0], self.marks[-1]
        return (s1 - s0) / (t1 - t0) if t1 > t0 else None


def train_and_evaluate(model, train_input_fn, eval_input_fn, max_steps: int,
                       clock: Callable[[], float] = time.monotonic) -> List[Tuple[int, dict]]:
    """``tf.estimator.train_and_evaluate`` as train.py:69-87 sets it up: train up to
    ``max_steps`` global steps in chunks that end at each checkpoint (``save_checkpoints_steps``);
    after a checkpoint, evaluate ``num_evaluation_steps`` batches if at least
    ``eval_start_delay_secs`` have passed since the start and ``eval_throttle_secs`` since the
    last evaluation; always evaluate once at the end.  Returns [(global step, metrics)]."""
    opt = model._run_option
    every = int(opt("save_checkpoints_steps") or 0)
    n_eval = int(opt("num_evaluation_steps") or 1)
    delay = float(opt("eval_start_delay_secs") or 0)
    throttle = float(opt("eval_throttle_secs") or 0)
    start = clock()
    last_eval = None
    results: List[Tuple[int, dict]] = []
    it = iter(train_input_fn())                    # one pass over the data, across the chunks
    step = int(model._host_step)
    while step < max_steps:
        nxt = min(max_steps, (step // every + 1) * every) if every > 0 else max_steps
        model.train(lambda: it, nxt - step)
        step = int(model._host_step)
        now = clock()
        due = now - start >= delay and (last_eval is None or now - last_eval >= throttle)
        if step >= max_steps or due:
            results.append((step, model.evaluate(eval_input_fn, n_eval)))
            last_eval = clock()
    if not results or results[-1][0] != step:
        results.append((step, model.evaluate(eval_input_fn, n_eval)))
    return results
