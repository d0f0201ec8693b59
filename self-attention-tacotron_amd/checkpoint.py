"""Checkpoints: one name-keyed ``model.ckpt-<global_step>.npz`` per save, written off the
training thread, restored in place.

The reference saves and restores through ``tf.estimator`` (train.py:67-79: ``RunConfig`` with
``save_checkpoints_steps`` / ``keep_checkpoint_max`` and a ``WarmStartSettings``); an Estimator
restores the newest checkpoint of ``model_dir`` before it trains, evaluates or predicts.  Here:

* the training state -- parameters, both Adam moments, BatchNorm moving statistics, global step,
  Philox seed and the guard's status words -- is copied device-to-device into ONE staging arena
  between steps, digested on the device (``sat_arena_digest``), copied to pinned host memory on
  a side stream and written by one writer thread (``Snapshotter``); the training thread never
  waits for the device;
* the file is keyed by TF variable name in TF layout (``Layout.unpack``), so it survives a
  change of the flat layout and can be filtered by regex (warm start);
* a load validates the whole file on the host against the model's ``Layout`` before any device
  tensor is touched, uploads into the staging arena, recomputes the digest on the device and
  only then copies into the live arenas (``copy_``: addresses never change, captured graphs stay
  valid).

File entries: ``var/<name>``, ``adam_m/<name>``, ``adam_v/<name>``, ``bn/<scope>/moving_mean``
/ ``moving_variance``, ``global_step``, ``rng_seed``, ``status`` and ``meta`` (JSON bytes: format
version, hparams, tensor manifest, digest, world size).
"""

from __future__ import annotations

import io
import json
import os
import re
import threading
import time
import zipfile
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np

from . import params as PR

FORMAT = "sat_amd.checkpoint"
FORMAT_VERSION = 1
PREFIX = "model.ckpt-"
_NAME = re.compile(r"^model\.ckpt-(\d+)\.npz$")
_M64 = (1 << 64) - 1


class CheckpointError(RuntimeError):
    """A checkpoint could not be written, read or applied; nothing was half-applied."""


# ------------------------------------------------------------------------------ digest (host)
_G = np.uint64(0x9E3779B97F4A7C15)
_C1 = np.uint64(0xBF58476D1CE4E5B9)
_C2 = np.uint64(0x94D049BB133111EB)


def _words(array) -> np.ndarray:
    a = np.ascontiguousarray(array)
    if a.dtype.itemsize % 4:
        raise ValueError(f"digest_host: 4- or 8-byte elements expected, got dtype {a.dtype}")
    return a.reshape(-1).view(np.uint32)


def digest_host(array, base_index: int = 0, chunk: int = 1 << 20) -> Tuple[int, int]:
    """(digest, non-finite count) of ``array`` read as 32-bit words: the numpy restatement of
    ``sat_arena_digest`` (include/sat_abi.h), uint64 wraparound arithmetic.  The count is of
    words whose fp32 exponent field is all ones (inf and NaN)."""
    w = _words(array)
    dig, bad = 0, 0
    for lo in range(0, w.size, chunk):
        c = w[lo:lo + chunk]
        pos = np.arange(lo + 1, lo + 1 + c.size, dtype=np.uint64) + np.uint64(base_index & _M64)
        z = (pos * _G) ^ c.astype(np.uint64)
        z = (z ^ (z >> np.uint64(30))) * _C1
        z = (z ^ (z >> np.uint64(27))) * _C2
        z ^= z >> np.uint64(31)
        dig = (dig + int(z.sum(dtype=np.uint64))) & _M64
        bad += int(np.count_nonzero((c & np.uint32(0x7F800000)) == np.uint32(0x7F800000)))
    return dig, bad


# ------------------------------------------------------------------------------ state layout
class StateLayout:
    """Word offsets of the training state inside one staging arena of 32-bit words:
    ``[params | adam_m | adam_v | bn | global_step (2) | rng_seed (2) | status (2) | digest out]``
    -- the float part first (digested with the non-finite count), the integer scalars chained
    behind it by ``base_index``.  The digest output (four uint64) rides at the end so one
    device-to-host copy carries everything."""

    def __init__(self, hp, layout: Optional[PR.Layout] = None):
        self.layout = layout if layout is not None else PR.Layout(PR.param_specs(hp))
        self.bn_names = PR.bn_buffer_names(hp)
        self.n_p = self.layout.total
        self.n_ch = sum(ch for _, ch in self.bn_names)
        self.n_bn = 2 * self.n_ch
        self.o_m, self.o_v, self.o_bn = self.n_p, 2 * self.n_p, 3 * self.n_p
        self.n_f = 3 * self.n_p + self.n_bn              # float words (even)
        self.o_gs, self.o_seed, self.o_status = self.n_f, self.n_f + 2, self.n_f + 4
        self.n_words = self.n_f + 6                      # digested words
        self.o_out = self.n_words                        # 4 x uint64, 8-byte aligned
        self.total = (self.n_words + 8 + 3) // 4 * 4

    def manifest(self) -> List[list]:
        out = [[f"var/{p.name}", list(p.shape)] for p in self.layout.specs]
        for scope, ch in self.bn_names:
            out.append([f"bn/{scope}/moving_mean", [ch]])
            out.append([f"bn/{scope}/moving_variance", [ch]])
        return out

    # ---- host arena <-> name-keyed entries
    def entries(self, arena: np.ndarray) -> Dict[str, np.ndarray]:
        """Name-keyed TF-layout arrays of a host staging arena (float32 view of the words)."""
        f = arena.view(np.float32)
        out: Dict[str, np.ndarray] = {}
        for kind, off in (("var", 0), ("adam_m", self.o_m), ("adam_v", self.o_v)):
            for k, v in self.layout.unpack(f[off:off + self.n_p]).items():
                out[f"{kind}/{k}"] = v
        o = self.o_bn
        for scope, ch in self.bn_names:
            out[f"bn/{scope}/moving_mean"] = f[o:o + ch]
            out[f"bn/{scope}/moving_variance"] = f[o + self.n_ch:o + self.n_ch + ch]
            o += ch
        i = arena.view(np.int32)
        out["global_step"] = i[self.o_gs:self.o_gs + 2].view(np.int64).copy()
        out["rng_seed"] = i[self.o_seed:self.o_seed + 2].view(np.int64).copy()
        out["status"] = i[self.o_status:self.o_status + 2].copy()
        return out

    def arena(self, entries: Dict[str, np.ndarray]) -> np.ndarray:
        """Inverse of ``entries``: a float32 array of ``total`` words (digest slots zero)."""
        a = np.zeros(self.total, np.float32)
        for kind, off in (("var", 0), ("adam_m", self.o_m), ("adam_v", self.o_v)):
            vals = {p.name: entries[f"{kind}/{p.name}"] for p in self.layout.specs}
            a[off:off + self.n_p] = self.layout.pack(vals)
        o = self.o_bn
        for scope, ch in self.bn_names:
            a[o:o + ch] = entries[f"bn/{scope}/moving_mean"]
            a[o + self.n_ch:o + self.n_ch + ch] = entries[f"bn/{scope}/moving_variance"]
            o += ch
        i = a.view(np.int32)
        i[self.o_gs:self.o_gs + 2] = np.asarray(entries["global_step"], np.int64).view(np.int32)
        i[self.o_seed:self.o_seed + 2] = np.asarray(entries["rng_seed"], np.int64).view(np.int32)
        i[self.o_status:self.o_status + 2] = np.asarray(entries["status"], np.int32)
        return a

    def digest(self, arena: np.ndarray) -> Tuple[int, int]:
        """The file's digest pair of a host arena: floats (counted) chained with the scalars."""
        w = arena.view(np.uint32)
        d0, bad = digest_host(w[:self.n_f])
        d1, _ = digest_host(w[self.n_f:self.n_words], base_index=self.n_f)
        return (d0 + d1) & _M64, bad


def initial_entries(hp, values: Dict[str, np.ndarray], bn: Dict[str, np.ndarray],
                    global_step: int = 0, rng_seed: int = 0) -> Dict[str, np.ndarray]:
    """Entries of an untrained state (``params.init_params`` / ``init_bn_buffers``): zero
    moments, clean status."""
    out: Dict[str, np.ndarray] = {}
    for k, v in values.items():
        v = np.asarray(v, np.float32)
        out[f"var/{k}"] = v
        out[f"adam_m/{k}"] = np.zeros_like(v)
        out[f"adam_v/{k}"] = np.zeros_like(v)
    for k, v in bn.items():
        out[f"bn/{k}"] = np.asarray(v, np.float32)
    out["global_step"] = np.array([global_step], np.int64)
    out["rng_seed"] = np.array([rng_seed], np.int64)
    out["status"] = np.zeros(2, np.int32)
    return out


# ------------------------------------------------------------------------------ files
def checkpoint_path(model_dir: str, step: int) -> str:
    return os.path.join(model_dir, f"{PREFIX}{int(step)}.npz")


def _hparams_json(hp) -> dict:
    vals = hp.values() if hasattr(hp, "values") else dict(hp or {})
    return json.loads(json.dumps(vals, default=str))


def _fsync_dir(d: str) -> None:
    try:
        fd = os.open(d, os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


def write_entries(path: str, entries: Dict[str, np.ndarray], meta: dict,
                  _savez=np.savez) -> str:
    """``entries`` + ``meta`` as one uncompressed .npz at ``path``: written under a temporary
    name in the same directory, fsynced, renamed.  Any failure removes the temporary file and
    raises ``CheckpointError``; no ``model.ckpt-*`` name exists before the rename."""
    d = os.path.dirname(os.path.abspath(path))
    tmp = os.path.join(d, f".tmp-{os.getpid()}-{threading.get_ident()}-{os.path.basename(path)}")
    blob = np.frombuffer(json.dumps(meta).encode("utf-8"), np.uint8)
    try:
        os.makedirs(d, exist_ok=True)
        with open(tmp, "wb") as f:
            _savez(f, meta=blob, **entries)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
        _fsync_dir(d)
    except BaseException as e:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        if isinstance(e, Exception):
            raise CheckpointError(f"writing {path} failed: {type(e).__name__}: {e}") from e
        raise
    return path


def list_checkpoints(model_dir: str) -> List[Tuple[int, str]]:
    """(step, path) of every ``model.ckpt-<step>.npz`` name in ``model_dir``, oldest first."""
    if not model_dir or not os.path.isdir(model_dir):
        return []
    out = []
    for n in os.listdir(model_dir):
        m = _NAME.match(n)
        if m:
            out.append((int(m.group(1)), os.path.join(model_dir, n)))
    return sorted(out)


def prune(model_dir: str, keep_max: Optional[int]) -> List[str]:
    """Remove the oldest files beyond ``keep_max`` (None / <= 0 keeps all, as tf.train.Saver)."""
    if not keep_max or keep_max <= 0:
        return []
    gone = []
    files = list_checkpoints(model_dir)
    for _, p in files[:max(0, len(files) - int(keep_max))]:
        try:
            os.unlink(p)
            gone.append(p)
        except OSError:
            pass
    return gone


def _refuse_tf(path: str) -> None:
    base = os.path.basename(path)
    tf_like = (os.path.exists(path + ".index") or os.path.exists(path + ".meta")
               or base == "checkpoint" or re.search(r"\.(index|meta|data-\d+-of-\d+)$", base))
    if os.path.isdir(path):
        tf_like = tf_like or os.path.exists(os.path.join(path, "checkpoint"))
    if tf_like:
        raise CheckpointError(
            f"{path} is a TF checkpoint (TensorFlow format): this build reads only its own "
            f"{PREFIX}<step>.npz files; convert the variables to that name-keyed format first")


def read_meta(path: str) -> dict:
    """The ``meta`` record of a checkpoint file; ``CheckpointError`` when the file is truncated,
    unreadable or not one of ours."""
    _refuse_tf(path)
    try:
        with np.load(path, allow_pickle=False) as z:
            if not hasattr(z, "files") or "meta" not in z.files:
                raise CheckpointError(f"{path}: not a {FORMAT} file (no meta record)")
            meta = json.loads(bytes(np.asarray(z["meta"], np.uint8)).decode("utf-8"))
    except CheckpointError:
        raise
    except Exception as e:
        raise CheckpointError(f"{path}: unreadable or truncated checkpoint "
                              f"({type(e).__name__}: {e})") from e
    if not isinstance(meta, dict) or meta.get("format") != FORMAT:
        raise CheckpointError(f"{path}: not a {FORMAT} file")
    if int(meta.get("version", -1)) > FORMAT_VERSION:
        raise CheckpointError(f"{path}: format version {meta.get('version')} is newer than "
                              f"this build's {FORMAT_VERSION}")
    return meta


def read_entries(path: str, prefixes: Optional[Iterable[str]] = None
                 ) -> Tuple[Dict[str, np.ndarray], dict]:
    """(entries, meta) of a checkpoint file (only entries under ``prefixes`` when given)."""
    meta = read_meta(path)
    pre = tuple(prefixes) if prefixes is not None else None
    try:
        with np.load(path, allow_pickle=False) as z:
            ent = {k: z[k] for k in z.files
                   if k != "meta" and (pre is None or k.startswith(pre))}
    except Exception as e:
        raise CheckpointError(f"{path}: unreadable or truncated checkpoint "
                              f"({type(e).__name__}: {e})") from e
    return ent, meta


def latest_checkpoint(model_dir: Optional[str]) -> Optional[str]:
    """The highest-step ``model.ckpt-<step>.npz`` of ``model_dir`` whose meta parses (a
    truncated or foreign file is skipped), or None."""
    for _, p in reversed(list_checkpoints(model_dir)):
        try:
            read_meta(p)
            return p
        except CheckpointError:
            continue
    return None


def check_manifest(sl: StateLayout, entries: Dict[str, np.ndarray], meta: dict, path: str,
                   kinds=("var", "adam_m", "adam_v", "bn")) -> None:
    """The file's tensors against the model's layout: a missing tensor, an extra tensor or a
    wrong shape raises ``CheckpointError`` naming it."""
    want = {n: tuple(s) for n, s in sl.manifest()}
    full = dict(want)
    for n, s in want.items():
        if n.startswith("var/"):
            full["adam_m/" + n[4:]] = s
            full["adam_v/" + n[4:]] = s
    full = {n: s for n, s in full.items() if n.split("/", 1)[0] in kinds}
    listed = {n: tuple(s) for n, s in meta.get("manifest", [])}
    for n, s in full.items():
        if n not in entries:
            raise CheckpointError(f"{path}: tensor {n} is missing (the model needs shape {s})")
        if tuple(entries[n].shape) != s or (n in listed and listed[n] != s):
            raise CheckpointError(f"{path}: tensor {n} has shape {tuple(entries[n].shape)}, "
                                  f"the model needs {s}")
        if entries[n].dtype != np.float32:
            raise CheckpointError(f"{path}: tensor {n} has dtype {entries[n].dtype}, not float32")
    for n in entries:
        if "/" in n and n.split("/", 1)[0] in kinds and n not in full:
            raise CheckpointError(f"{path}: tensor {n} is not a tensor of this model")
    if set(kinds) >= {"var", "adam_m", "adam_v", "bn"}:
        for n, shape, dt in (("global_step", (1,), np.int64), ("rng_seed", (1,), np.int64),
                             ("status", (2,), np.int32)):
            if n not in entries or tuple(entries[n].shape) != shape or entries[n].dtype != dt:
                raise CheckpointError(f"{path}: scalar record {n} is missing or malformed")


class Loaded:
    """A validated checkpoint on the host: the staging arena (float32 words), its digest pair
    and the file's meta."""

    def __init__(self, path, arena, digest, meta):
        self.path, self.arena, self.digest, self.meta = path, arena, digest, meta


def load(path: str, sl: StateLayout) -> Loaded:
    """Read and validate ``path`` against ``sl`` entirely on the host.  The file's stored digest
    is the one the device check after the upload compares against; when the file was written
    under the same flat layout it must also equal the host arena's own digest."""
    ent, meta = read_entries(path)
    check_manifest(sl, ent, meta, path)
    arena = sl.arena(ent)
    dig = meta.get("digest")
    same_layout = meta.get("manifest") == sl.manifest() and meta.get("n_words") == sl.n_words
    if same_layout and dig is not None:
        digest = (int(dig[0]), int(dig[1]))
    else:                                   # another flat layout wrote it: digest of ours
        digest = sl.digest(arena)
    if digest[1] != 0:
        raise CheckpointError(f"{path}: records {digest[1]} non-finite value(s)")
    return Loaded(path, arena, digest, meta)


def select_vars(names: Iterable[str], regexes: Iterable[str]) -> List[str]:
    """Variable names matched by any of ``regexes`` (``re.match`` from the start of the name, as
    TF's ``vars_to_warm_start``); a regex that matches nothing raises."""
    names = list(names)
    picked, seen = [], set()
    for rx in ([regexes] if isinstance(regexes, str) else list(regexes)):
        hit = [n for n in names if re.match(rx, n)]
        if not hit:
            raise CheckpointError(f"vars_to_warm_start regex {rx!r} matches no variable")
        for n in hit:
            if n not in seen:
                seen.add(n)
                picked.append(n)
    return picked


def load_warm_start(path: str, sl: StateLayout, regexes) -> Dict[str, np.ndarray]:
    """{variable name: TF-layout array} of the ``var/*`` entries of ``path`` matched by
    ``regexes``, shapes checked against the model.  No moments, no BN statistics, no step."""
    ent, meta = read_entries(path, prefixes=("var/",))
    have = [n[4:] for n in ent]
    picked = select_vars(have, regexes)
    out = {}
    for n in picked:
        if n not in sl.layout.shapes:
            raise CheckpointError(f"{path}: tensor var/{n} is not a tensor of this model")
        a = ent["var/" + n]
        if tuple(a.shape) != tuple(sl.layout.shapes[n]) or a.dtype != np.float32:
            raise CheckpointError(f"{path}: tensor var/{n} has shape {tuple(a.shape)} "
                                  f"{a.dtype}, the model needs {tuple(sl.layout.shapes[n])} "
                                  "float32")
        if not np.isfinite(a).all():
            raise CheckpointError(f"{path}: tensor var/{n} holds non-finite values")
        out[n] = a
    return out


def save_arena(model_dir: str, arena: np.ndarray, sl: StateLayout, hp, digest: Tuple[int, int],
               world: int = 1, keep_max: Optional[int] = None, path: Optional[str] = None,
               _savez=np.savez) -> str:
    """Write one checkpoint from a host staging arena and prune ``model_dir``."""
    ent = sl.entries(arena)
    step = int(ent["global_step"][0])
    meta = {"format": FORMAT, "version": FORMAT_VERSION, "global_step": step,
            "hparams": _hparams_json(hp), "manifest": sl.manifest(), "n_words": sl.n_words,
            "digest": [int(digest[0]), int(digest[1])], "world_size": int(world)}
    path = path or checkpoint_path(model_dir, step)
    write_entries(path, ent, meta, _savez=_savez)
    if keep_max and _NAME.match(os.path.basename(path)):
        prune(os.path.dirname(os.path.abspath(path)), keep_max)
    return path


# ------------------------------------------------------------------------------ device side
class Snapshotter:
    """The device half of a Trainer's checkpoints: ONE staging arena on the device, its pinned
    host mirror, a side stream and ONE writer thread.

    ``snapshot()`` enqueues, on the current stream and outside any capture, the device-to-device
    copies of the state into the staging arena and its digest; the side stream then copies the
    arena to pinned memory behind an event, followed by a sequence word the writer thread polls
    in pinned memory (it makes no device API call, so a graph capture on the training thread is
    never disturbed).  The training thread does not synchronise.  A snapshot that finds
    non-finite values, a non-zero ``status[0]``, replicas that disagree or an I/O error leaves no
    file; the error is raised from the next ``snapshot()`` / ``wait()``."""

    def __init__(self, trainer, verify_host: bool = True):
        import torch
        self.t = trainer
        m = trainer.m
        self.sl = sl = StateLayout(m.hp, m.layout)
        if m.params.numel() != sl.n_p or m.bn.buf.numel() != sl.n_bn:
            raise CheckpointError("state layout does not match the engine's arenas")
        dev = m.device
        self.stage = torch.zeros(sl.total, dtype=torch.float32, device=dev)
        self.host = torch.zeros(sl.total, dtype=torch.float32, pin_memory=True)
        self.seq = torch.zeros(2, dtype=torch.int32, device=dev)
        self.seq_host = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        self._seq_np = self.seq_host.numpy()
        self._host_np = self.host.numpy()
        self.count = 0
        self.side = torch.cuda.Stream(device=dev)
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="sat-ckpt")
        self.future = None
        self.verify_host = bool(verify_host)
        self.last_path: Optional[str] = None
        self.last_digest: Optional[Tuple[int, int]] = None
        self._gath = self._gath_host = None
        # the writer's poll gives up after this long, when close() cancels it, or once the
        # main thread has ended (interpreter exit never waits on a copy that will not land)
        self.timeout_s = 120.0
        self._cancel = threading.Event()

    # views of the staging arena
    def _i64(self, off: int, n: int = 1):
        import torch
        return self.stage[off:off + 2 * n].view(torch.int64)

    def _i32(self, off: int, n: int):
        import torch
        return self.stage[off:off + n].view(torch.int32)

    def _digest_stage(self) -> None:
        """The four uint64 output words: [0:2] digest / non-finite count of the float words,
        [2] the rank's error flag (set by snapshot(); gathered with [0:2] under data
        parallelism), [3] digest of the scalar words chained at base_index n_f (the file's
        digest is [0] + [3] mod 2^64)."""
        from . import _lib
        from . import kernels as K
        sl = self.sl
        K.fill_(self._i32(sl.o_out, 8), 0)
        base = self.stage.data_ptr()
        out = base + 4 * sl.o_out
        _lib.call("sat_arena_digest", base, sl.n_f, 0, 1, out, K._stream())
        _lib.call("sat_arena_digest", base + 4 * sl.n_f, sl.n_words - sl.n_f, sl.n_f, 0,
                  out + 24, K._stream())

    def _exchanging(self, force: bool) -> bool:
        from . import dp
        t = self.t
        return t.world > 1 or ((force or t.force_exchange) and dp.is_distributed(t.pg))

    def snapshot(self, model_dir: Optional[str] = None, keep_max: Optional[int] = None,
                 path: Optional[str] = None, force_exchange: bool = False) -> None:
        import torch
        from . import dp
        if model_dir is None and path is None:
            raise ValueError("snapshot: model_dir or path needed")
        # one staging arena, no queue: wait for the previous snapshot.  What it raised is
        # re-raised only AFTER this call's collective, so that under data parallelism a rank
        # with an error (an I/O error on rank 0, say) never leaves the others alone inside the
        # all-gather; its flag travels in the gathered words and the other ranks raise too.
        err = None
        try:
            self.wait()
        except CheckpointError as e:
            err = e
        t, sl, st = self.t, self.sl, self.stage
        st[:sl.n_p].copy_(t.m.params)
        st[sl.o_m:sl.o_m + sl.n_p].copy_(t.exp_avg)
        st[sl.o_v:sl.o_v + sl.n_p].copy_(t.exp_avg_sq)
        st[sl.o_bn:sl.o_bn + sl.n_bn].copy_(t.m.bn.buf)
        self._i64(sl.o_gs).copy_(t.global_step)
        self._i64(sl.o_seed).copy_(t.seed)
        self._i32(sl.o_status, 2).copy_(t.status)
        self._digest_stage()
        exchanging = self._exchanging(force_exchange)
        world = dp.world_size(t.pg)
        if exchanging:
            # replica drift: every rank's {float digest, non-finite count} (16 bytes) and its
            # error flag -- the ONE collective of a snapshot, entered by every rank
            import torch.distributed as tdist
            if err is not None:
                self._i64(sl.o_out + 4).fill_(1)
            if self._gath is None or self._gath.numel() != 3 * world:
                self._gath = torch.zeros(3 * world, dtype=torch.int64, device=st.device)
                self._gath_host = torch.zeros(3 * world, dtype=torch.int64, pin_memory=True)
            tdist.all_gather_into_tensor(self._gath, self._i64(sl.o_out, 3), group=t.pg)
        if err is not None:
            raise err
        self.count += 1
        self.seq.fill_(self.count)
        writes = dp.rank(t.pg) == 0
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ready)
            lo = 0 if writes else sl.n_f
            self.host[lo:].copy_(st[lo:], non_blocking=True)
            if exchanging:
                self._gath_host.copy_(self._gath, non_blocking=True)
            self.seq_host.copy_(self.seq, non_blocking=True)      # last: the writer's signal
        self.future = self.pool.submit(self._write, self.count, model_dir, keep_max, path,
                                       writes, world if exchanging else 0, world)

    def _write(self, count, model_dir, keep_max, path, writes, gathered, world):
        t0 = time.monotonic()
        while int(self._seq_np[0]) != count:
            if (time.monotonic() - t0 > self.timeout_s or self._cancel.is_set()
                    or not threading.main_thread().is_alive()):
                raise CheckpointError("snapshot: the device-to-host copy did not arrive")
            time.sleep(0.0005)
        sl, a = self.sl, self._host_np
        out = a[sl.o_out:sl.o_out + 8].view(np.uint64)
        d_float, bad, d_scal = int(out[0]), int(out[1]), int(out[3])
        digest = ((d_float + d_scal) & _M64, bad)
        status = a.view(np.int32)[sl.o_status:sl.o_status + 2]
        if bad:
            raise CheckpointError(f"snapshot refused: {bad} non-finite value(s) in the "
                                  "parameters, Adam moments or BatchNorm statistics")
        if int(status[0]) != 0:
            raise CheckpointError(f"snapshot refused: {int(status[0])} training step(s) skipped "
                                  f"by the health guard (first error code {int(status[1])})")
        if gathered:
            g = self._gath_host.numpy().view(np.uint64).reshape(gathered, 3)
            failed = [r for r in range(gathered) if int(g[r, 2]) != 0]
            if failed:
                raise CheckpointError(f"snapshot refused: the previous snapshot failed on "
                                      f"rank(s) {failed}")
            if not (g[:, :2] == g[0, :2]).all():
                raise CheckpointError(
                    "snapshot refused: data-parallel replicas differ (float-state digests "
                    + ", ".join(f"{int(x):#018x}" for x in g[:, 0]) + ")")
        self.last_digest = digest
        if not writes:
            # every rank reports the file rank 0 writes, so what follows a snapshot (whether a
            # later evaluate() restores) is decided alike on all of them
            step = int(a.view(np.int32)[sl.o_gs:sl.o_gs + 2].view(np.int64)[0])
            self.last_path = path or checkpoint_path(model_dir, step)
            return self.last_path
        if self.verify_host and sl.digest(a) != digest:
            raise CheckpointError("snapshot refused: the host copy's digest differs from the "
                                  "device's (corrupt device-to-host transfer)")
        p = save_arena(model_dir, a, sl, self.t.hp, digest, world=world, keep_max=keep_max,
                       path=path)
        self.last_path = p
        return p

    def wait(self) -> Optional[str]:
        """Block until the pending snapshot's file is on disk; raise what it raised."""
        f, self.future = self.future, None
        if f is None:
            return self.last_path
        return f.result()

    # ---- restore
    def upload_verified(self, ck: Loaded) -> None:
        """Host arena -> staging arena, then the device digest against the file's.  The live
        arenas are not touched here."""
        import torch
        self.wait()
        sl = self.sl
        self._host_np[:] = ck.arena
        self.stage.copy_(self.host, non_blocking=True)
        self._digest_stage()
        out = self._i64(sl.o_out, 4).cpu().numpy().view(np.uint64)
        got = ((int(out[0]) + int(out[3])) & _M64, int(out[1]))
        if got != tuple(ck.digest):
            raise CheckpointError(
                f"{ck.path}: digest after upload {got[0]:#018x} (non-finite {got[1]}) differs "
                f"from the file's {ck.digest[0]:#018x}; the model was left untouched")

    def apply_stage(self, seed_offset: int = 0) -> None:
        """Staging arena -> the live arenas, in place."""
        t, sl, st = self.t, self.sl, self.stage
        t.m.params.copy_(st[:sl.n_p])
        t.exp_avg.copy_(st[sl.o_m:sl.o_m + sl.n_p])
        t.exp_avg_sq.copy_(st[sl.o_v:sl.o_v + sl.n_p])
        t.m.bn.buf.copy_(st[sl.o_bn:sl.o_bn + sl.n_bn])
        t.global_step.copy_(self._i64(sl.o_gs))
        t.seed.copy_(self._i64(sl.o_seed))
        if seed_offset:
            t.seed.add_(int(seed_offset))
        t.status.copy_(self._i32(sl.o_status, 2))

    def close(self) -> None:
        self._cancel.set()
        try:
            self.wait()
        finally:
            self.pool.shutdown(wait=True)


def stage_verified(ck: Loaded, sl: StateLayout, device):
    """The arena of ``ck`` in a temporary device buffer whose device digest equals the file's
    (``CheckpointError`` otherwise); no live tensor is touched."""
    import torch
    from . import kernels as K
    stage = torch.from_numpy(ck.arena).to(device)
    out = torch.zeros(8, dtype=torch.int32, device=device)
    K.fill_(out, 0)
    device_digest(stage[:sl.n_f], 0, True, out=out[:4])
    device_digest(stage[sl.n_f:sl.n_words], sl.n_f, False, out=out[4:])
    w = out.cpu().numpy().view(np.uint64)
    got = ((int(w[0]) + int(w[2])) & _M64, int(w[1]))
    if got != tuple(ck.digest):
        raise CheckpointError(
            f"{ck.path}: digest after upload {got[0]:#018x} (non-finite {got[1]}) differs from "
            f"the file's {ck.digest[0]:#018x}; the model was left untouched")
    return stage


def upload_to_engine(ck: Loaded, sl: StateLayout, engine) -> None:
    """Restore of a model that has no Trainer yet: the arena goes to a temporary device buffer,
    its device digest is compared with the file's, then parameters and BatchNorm statistics are
    copied into the engine's arenas in place.  The optimiser state stays pending on the host."""
    stage = stage_verified(ck, sl, engine.device)
    engine.params.copy_(stage[:sl.n_p])
    engine.bn.buf.copy_(stage[sl.o_bn:sl.o_bn + sl.n_bn])


def device_digest(tensor, base_index: int = 0, count_nonfinite: bool = True,
                  out=None) -> Optional[Tuple[int, int]]:
    """(digest, non-finite count) of a contiguous device tensor of 4-byte (or 8-byte) elements
    through ``sat_arena_digest``; synchronises (a test / tool helper, not on the step path)."""
    import torch
    from . import _lib
    from . import kernels as K
    if not tensor.is_cuda or not tensor.is_contiguous() or tensor.element_size() % 4:
        raise ValueError("device_digest: contiguous device tensor of 4- or 8-byte elements")
    n = tensor.numel() * tensor.element_size() // 4
    fresh = out is None
    if fresh:
        out = torch.zeros(4, dtype=torch.int32, device=tensor.device)
        K.fill_(out, 0)
    _lib.call("sat_arena_digest", tensor.data_ptr() if n else 0, n, int(base_index),
              1 if count_nonfinite else 0, out.data_ptr(), K._stream())
    if not fresh:
        return None
    w = out.cpu().numpy().view(np.uint64)
    return int(w[0]), int(w[1])
