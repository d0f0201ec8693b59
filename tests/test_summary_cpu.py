"""Training summaries, host side (sat_amd/summary.py): the event-file format read back with the
package's own TFRecord / protobuf readers, the PNG encoder against a stdlib decoder, the writer
thread's error path and the train_and_evaluate schedule under a fake clock."""
import os
import struct

import numpy as np
import pytest

import summary_ref as R


def _records(path):
    from sat_amd import tfrecord
    with open(path, "rb") as f:
        return tfrecord.split_records(f.read(), verify=True)


def test_event_file_round_trip(tmp_path):
    from sat_amd import summary as S
    from sat_amd import tfrecord
    d = tmp_path / "run"
    w = S.EventFileWriter(str(d), clock=lambda: 1234567.5)
    vals = {"loss_with_teacher": np.float32(0.1234567), "learning_rate": np.float32(1e-30),
            "global_norm": np.float32(3.4e38)}
    w.add_scalars(2, vals)
    img = (np.arange(5 * 7, dtype=np.uint8) * 7).reshape(5, 7)
    w.add_deferred(3, lambda: (1234567.5, [S.image_value("alignment1/0", img)]))
    w.add_scalars(1 << 40, {"x": -0.0})
    w.close()
    files = os.listdir(d)
    assert len(files) == 1
    secs, host = files[0].split(".")[3], files[0].split(".", 4)[4]
    assert files[0].startswith("events.out.tfevents.1234567.") and host and secs == "1234567"
    recs = _records(os.path.join(d, files[0]))
    assert len(recs) == 4
    # the first record: wall time and the file version, nothing else
    first = {f: v for f, _, v in tfrecord._fields(recs[0])}
    assert first[3] == b"brain.Event:2" and set(first) == {1, 3}
    assert struct.unpack("<d", first[1])[0] == 1234567.5
    # steps and tags through the raw field reader
    steps, tags, floats = [], [], {}
    for rec in recs[1:]:
        ev = {f: v for f, _, v in tfrecord._fields(rec)}
        steps.append(ev[2])
        for f, wt, value in tfrecord._fields(ev[5]):
            assert (f, wt) == (1, 2)
            d2 = {f2: (wt2, v2) for f2, wt2, v2 in tfrecord._fields(value)}
            tag = d2[1][1].decode()
            tags.append(tag)
            if 2 in d2:
                assert d2[2][0] == 5                       # fixed32: a float
                floats[tag] = d2[2][1]
            if 4 in d2:
                im = {f3: v3 for f3, _, v3 in tfrecord._fields(d2[4][1])}
                assert (im[1], im[2], im[3]) == (5, 7, 1)
                assert (R.decode_png(im[4]) == img).all()
    assert steps == [2, 3, 1 << 40]
    assert tags == list(vals) + ["alignment1/0", "x"]
    for k, v in vals.items():                              # bit-exact float32
        assert floats[k] == np.float32(v).tobytes()
    assert floats["x"] == np.float32(-0.0).tobytes()
    # and through the tests' event reader (used by the GPU tests)
    evs = R.read_events(os.path.join(d, files[0]))
    assert evs[0]["file_version"] == "brain.Event:2" and evs[1]["step"] == 2
    assert evs[1]["scalars"]["global_norm"] == np.float32(3.4e38)
    assert evs[2]["images"]["alignment1/0"][:2] == (5, 7)


def _pictures():
    rng = np.random.default_rng(0)
    yield np.zeros((1, 1), np.uint8)
    yield np.full((3, 1), 255, np.uint8)
    yield rng.integers(0, 256, size=(37, 33), dtype=np.uint8)
    yield np.tile(np.arange(256, dtype=np.uint8), (2, 3))


def test_png_decodes_to_the_input():
    from sat_amd import summary as S
    for a in _pictures():
        png = S.encode_png(a)
        assert png[:8] == b"\x89PNG\r\n\x1a\n"
        got = R.decode_png(png)
        assert got.shape == a.shape and (got == a).all()
    for bad in (np.zeros((2, 2), np.float32), np.zeros((0, 3), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            S.encode_png(bad)


def test_reference_decoder_handles_every_filter():
    """The decoder itself, on lines written with filters 1..4 (zlib + struct only)."""
    import zlib
    from sat_amd.summary import _chunk
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, size=(5, 9), dtype=np.uint8)
    raw = bytearray()
    prev = np.zeros(9, np.int32)
    for y, ft in enumerate((0, 1, 2, 3, 4)):
        cur = a[y].astype(np.int32)
        left = np.concatenate([[0], cur[:-1]])
        ul = np.concatenate([[0], prev[:-1]])
        pred = {0: np.zeros(9, np.int32), 1: left, 2: prev, 3: (left + prev) // 2,
                4: np.array([R._paeth(int(l), int(u), int(c)) for l, u, c in zip(left, prev, ul)])}
        raw += bytes([ft]) + ((cur - pred[ft]) & 0xFF).astype(np.uint8).tobytes()
        prev = cur
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 9, 5, 8, 0, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(bytes(raw))) + _chunk(b"IEND", b""))
    assert (R.decode_png(png) == a).all()


def test_png_opens_in_pil():
    Image = pytest.importorskip("PIL.Image")
    import io
    from sat_amd import summary as S
    for a in _pictures():
        im = Image.open(io.BytesIO(S.encode_png(a)))
        assert im.mode == "L" and im.size == (a.shape[1], a.shape[0])
        assert (np.asarray(im) == a).all()


def test_unwritable_directory_raises_at_the_next_call(tmp_path):
    from sat_amd import summary as S
    blocker = tmp_path / "file"
    blocker.write_bytes(b"x")
    w = S.EventFileWriter(str(blocker / "logs"))           # a directory under a regular file
    w.add_scalars(1, {"a": 1.0})                           # only queues
    w._q.join()
    with pytest.raises(S.SummaryError, match="NotADirectoryError|FileExistsError"):
        w.add_scalars(2, {"a": 2.0})
    w.add_scalars(3, {"a": 3.0})                           # fails again, reported by close()
    with pytest.raises(S.SummaryError):
        w.close()
    assert sorted(os.listdir(tmp_path)) == ["file"] and blocker.read_bytes() == b"x"
    # a writer that never got an event leaves nothing behind either
    S.EventFileWriter(str(tmp_path / "unused")).close()
    assert sorted(os.listdir(tmp_path)) == ["file"]


def test_reference_matches_a_hand_made_picture():
    """summary_ref.render on a 2 x 3 crop: the formula, the flip and the zero border."""
    src = np.array([[0.0, 1.0], [0.5, 0.25], [1.0, 0.0]], np.float32)     # [c][r], col_stride 2
    got = R.render(src, [0], [2], [3], 2, 3, 4)
    want = np.zeros((1, 3, 4), np.uint8)
    want[0, 0, :3] = [255, 64, 0]                          # source row 1 on top
    want[0, 1, :3] = [0, 128, 255]                         # source row 0 at the bottom
    assert (got == want).all()


class _FakeModel:
    """train() advances a fake clock by one second per step; records every call."""

    def __init__(self, every, delay, throttle, n_eval=2, start_step=0):
        self.opts = {"save_checkpoints_steps": every, "num_evaluation_steps": n_eval,
                     "eval_start_delay_secs": delay, "eval_throttle_secs": throttle}
        self._host_step = start_step
        self.now = 100.0
        self.calls = []

    def _run_option(self, name):
        return self.opts[name]

    def clock(self):
        return self.now

    def train(self, input_fn, steps):
        it = iter(input_fn())
        for _ in range(steps):
            next(it)
            self._host_step += 1
            self.now += 1.0
        self.calls.append(("train", steps))

    def evaluate(self, input_fn, steps):
        self.calls.append(("eval", self._host_step, steps))
        self.now += 3.0
        return {"loss": float(self._host_step), "global_step": self._host_step}


def _endless():
    while True:
        yield None, None


def test_train_and_evaluate_follows_the_schedule():
    from sat_amd import models
    # checkpoints every 10 steps = every 10 s; first evaluation no sooner than 25 s after the
    # start, then at most one per 20 s (an evaluation takes 3 s), and one at the end
    m = _FakeModel(every=10, delay=25, throttle=20)
    out = models.train_and_evaluate(m, _endless, _endless, 75, clock=m.clock)
    evals = [c[1] for c in m.calls if c[0] == "eval"]
    # t = 10, 20 (too early), 30 -> eval (ends t = 33), 43 (10 s later), 53 -> eval at 20 s
    # (ends 56), 66, 76 -> eval (20 s), then the last chunk of 5 steps and the final one
    assert evals == [30, 50, 70, 75]
    assert [s for s, _ in out] == evals and out[-1][1]["global_step"] == 75
    assert [c[1] for c in m.calls if c[0] == "train"] == [10] * 7 + [5]
    assert all(c[2] == 2 for c in m.calls if c[0] == "eval")
    # resuming mid-way: the first chunk ends at the next checkpoint step; no throttle, no delay
    m = _FakeModel(every=10, delay=0, throttle=0, start_step=14)
    models.train_and_evaluate(m, _endless, _endless, 32, clock=m.clock)
    assert [c[1] for c in m.calls if c[0] == "train"] == [6, 10, 2]
    assert [c[1] for c in m.calls if c[0] == "eval"] == [20, 30, 32]
    # nothing left to train: still one evaluation
    m = _FakeModel(every=10, delay=1e9, throttle=1e9, start_step=40)
    models.train_and_evaluate(m, _endless, _endless, 40, clock=m.clock)
    assert m.calls == [("eval", 40, 2)]
