"""Checkpoint format and host side (sat_amd/checkpoint.py) without a GPU: the numpy restatement
of ``sat_arena_digest``, the name-keyed file, ``latest_checkpoint``, pruning, the atomic write,
manifest checks and the warm-start filter."""
import json
import os

import numpy as np
import pytest

import _sat_path  # noqa: E402

_sat_path.load()
from sat_amd import checkpoint as C  # noqa: E402
from sat_amd import hparams, params  # noqa: E402

M64 = (1 << 64) - 1


def _mix(p, w):
    """include/sat_abi.h, in Python integers."""
    z = (((p + 1) * 0x9E3779B97F4A7C15) & M64) ^ w
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


FIXED = np.array([0, 1, 0x3F800000, 0xFFFFFFFF, 0x7F800000, 0x12345678, 0x80000000],
                 dtype=np.uint32)


def test_digest_host_known_answer():
    # computed once with Python integers from the header's definition of mix
    assert C.digest_host(FIXED) == (0x27BAF3AEB5EE0B32, 2)
    assert C.digest_host(FIXED, base_index=(1 << 33) + 5) == (0x335AA80335B870D7, 2)
    assert C.digest_host(FIXED) == (sum(_mix(i, int(w)) for i, w in enumerate(FIXED)) & M64, 2)
    assert C.digest_host(np.zeros(0, np.float32)) == (0, 0)
    # float32 and its bit pattern digest alike; int64 is read as two words per element
    f = np.array([1.0, -2.5, 3.25], np.float32)
    assert C.digest_host(f) == C.digest_host(f.view(np.uint32))
    q = np.array([7, -1], np.int64)
    assert C.digest_host(q) == C.digest_host(q.view(np.uint32))


def test_digest_depends_on_position():
    a = np.arange(1, 9, dtype=np.uint32)
    b = a.copy()
    b[[2, 5]] = b[[5, 2]]
    assert C.digest_host(a)[0] != C.digest_host(b)[0]
    assert C.digest_host(a)[0] != C.digest_host(a, base_index=1)[0]


def test_digest_chains_with_base_index():
    rng = np.random.default_rng(0)
    w = rng.integers(0, 1 << 32, size=1001, dtype=np.uint64).astype(np.uint32)
    whole = C.digest_host(w, base_index=11)
    lo, hi = C.digest_host(w[:400], base_index=11), C.digest_host(w[400:], base_index=411)
    assert ((lo[0] + hi[0]) & M64, lo[1] + hi[1]) == whole
    assert C.digest_host(w, chunk=97) == C.digest_host(w)


def test_nonfinite_count():
    a = np.array([1.0, np.inf, 0.5, np.nan, 1e-45, -0.0], np.float32)   # 1e-45: a denormal
    assert C.digest_host(a)[1] == 2
    assert C.digest_host(np.array([-np.inf], np.float32))[1] == 1


@pytest.fixture(scope="module")
def state():
    hp = hparams.ljspeech_hparams()
    sl = C.StateLayout(hp)
    vals = params.init_params(hp, seed=3)
    ent = C.initial_entries(hp, vals, params.init_bn_buffers(hp), global_step=12, rng_seed=99)
    rng = np.random.default_rng(1)
    for k in list(ent):
        if k.startswith(("adam_", "bn/")):
            ent[k] = rng.standard_normal(ent[k].shape).astype(np.float32)
    return hp, sl, ent, sl.arena(ent)


def _save(tmp, state, step=None, **kw):
    hp, sl, ent, arena = state
    a = arena
    if step is not None:
        a = arena.copy()
        a.view(np.int32)[sl.o_gs:sl.o_gs + 2] = np.array([step], np.int64).view(np.int32)
    return C.save_arena(str(tmp), a, sl, hp, sl.digest(a), **kw)


def test_named_file_round_trips_bit_for_bit(tmp_path, state):
    hp, sl, ent, arena = state
    path = _save(tmp_path, state)
    assert os.path.basename(path) == "model.ckpt-12.npz"
    got, meta = C.read_entries(path)
    assert set(got) == set(ent)
    for k, v in ent.items():
        assert got[k].dtype == np.asarray(v).dtype and got[k].shape == np.asarray(v).shape, k
        assert got[k].tobytes() == np.asarray(v).tobytes(), k
    # TF layout under TF names: an LSTM kernel is stored gate-blocked, not gate-interleaved
    k = "decoder/lstm1/kernel"
    assert np.array_equal(got["var/" + k], params.init_params(hp, seed=3)[k])
    assert meta["format"] == C.FORMAT and meta["global_step"] == 12 and meta["world_size"] == 1
    assert meta["hparams"]["outputs_per_step"] == hp.outputs_per_step
    assert meta["manifest"] == sl.manifest()
    ck = C.load(path, sl)
    assert ck.arena.tobytes() == arena.tobytes()
    assert ck.digest == sl.digest(arena) == tuple(meta["digest"])
    # uncompressed
    import zipfile
    with zipfile.ZipFile(path) as z:
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())


def test_latest_checkpoint_skips_a_truncated_file(tmp_path, state):
    assert C.latest_checkpoint(str(tmp_path)) is None
    assert C.latest_checkpoint(None) is None
    p5 = _save(tmp_path, state, step=5)
    p9 = _save(tmp_path, state, step=9)
    assert C.latest_checkpoint(str(tmp_path)) == p9
    blob = open(p9, "rb").read()
    open(p9, "wb").write(blob[:len(blob) // 2])
    assert C.latest_checkpoint(str(tmp_path)) == p5
    with pytest.raises(C.CheckpointError, match="truncated"):
        C.load(p9, state[1])
    # numeric, not lexical, order
    p10 = _save(tmp_path, state, step=10)
    assert C.latest_checkpoint(str(tmp_path)) == p10


def test_pruning_keeps_the_newest(tmp_path, state):
    for s in (1, 2, 3, 10, 20):
        _save(tmp_path, state, step=s, keep_max=3)
    assert [s for s, _ in C.list_checkpoints(str(tmp_path))] == [3, 10, 20]
    _save(tmp_path, state, step=30, keep_max=None)
    assert len(C.list_checkpoints(str(tmp_path))) == 4


def test_failed_write_leaves_no_file(tmp_path, state):
    def broken(f, **arrays):
        f.write(b"PK\x03\x04 half a file")
        raise OSError(28, "No space left on device")

    with pytest.raises(C.CheckpointError, match="No space left"):
        _save(tmp_path, state, _savez=broken)
    assert os.listdir(tmp_path) == []
    _save(tmp_path, state, step=4)
    with pytest.raises(C.CheckpointError):
        _save(tmp_path, state, step=8, keep_max=1, _savez=broken)
    assert os.listdir(tmp_path) == ["model.ckpt-4.npz"]     # nothing pruned, nothing left behind


def _rewrite(path, out, fn):
    ent, meta = C.read_entries(path)
    fn(ent, meta)
    return C.write_entries(str(out), ent, meta)


def test_manifest_mismatches_name_the_tensor(tmp_path, state):
    hp, sl, ent, arena = state
    path = _save(tmp_path, state)
    name = "decoder/attention1/query_layer/kernel"

    def drop(e, m):
        del e["adam_v/" + name]
    with pytest.raises(C.CheckpointError, match=f"adam_v/{name} is missing"):
        C.load(_rewrite(path, tmp_path / "a.npz", drop), sl)

    def extra(e, m):
        e["var/decoder/unknown/kernel"] = np.zeros(3, np.float32)
    with pytest.raises(C.CheckpointError, match="var/decoder/unknown/kernel is not a tensor"):
        C.load(_rewrite(path, tmp_path / "b.npz", extra), sl)

    def reshape(e, m):
        e["var/" + name] = e["var/" + name].T.copy()
    with pytest.raises(C.CheckpointError, match=f"var/{name} has shape"):
        C.load(_rewrite(path, tmp_path / "c.npz", reshape), sl)

    def bn(e, m):
        del e["bn/encoder/cbhg/proj1/bn/moving_variance"]
    with pytest.raises(C.CheckpointError, match="bn/encoder/cbhg/proj1/bn/moving_variance"):
        C.load(_rewrite(path, tmp_path / "d.npz", bn), sl)

    # a model with the transition agent has two tensors this file lacks
    hp2 = hparams.ljspeech_hparams(use_forward_attention_transition_agent=True)
    with pytest.raises(C.CheckpointError, match="transition_factor_projection/kernel is missing"):
        C.load(path, C.StateLayout(hp2))
    # ... and the file it writes still loads by name into the plain model's warm start
    sl2 = C.StateLayout(hp2)
    ent2 = C.initial_entries(hp2, params.init_params(hp2, seed=3), params.init_bn_buffers(hp2))
    a2 = sl2.arena(ent2)
    p2 = C.save_arena(str(tmp_path / "agent"), a2, sl2, hp2, sl2.digest(a2))
    got = C.load_warm_start(p2, sl, ["encoder/.*"])
    assert got and all(np.array_equal(v, ent["var/" + k]) for k, v in got.items())


def test_a_flipped_bit_fails_the_stored_digest(tmp_path, state):
    hp, sl, ent, arena = state
    path = _save(tmp_path, state)
    ck = C.load(path, sl)
    bad = ck.arena.copy()
    bad.view(np.uint32)[12345] ^= 1
    assert sl.digest(bad) != ck.digest


def test_warm_start_filter():
    names = [p.name for p in params.param_specs(hparams.ljspeech_hparams())]
    enc = C.select_vars(names, ["encoder/.*"])
    assert enc and all(n.startswith("encoder/") for n in enc)
    assert set(enc) == {n for n in names if n.startswith("encoder/")}
    assert "embedding" not in enc
    both = C.select_vars(names, ["embedding", "decoder/lstm[12]/.*", "embedding"])
    assert both == ["embedding", "decoder/lstm1/kernel", "decoder/lstm1/bias",
                    "decoder/lstm2/kernel", "decoder/lstm2/bias"]
    assert C.select_vars(names, [".*"]) == names
    assert C.select_vars(names, ".*bias") == [n for n in names if n.endswith("bias")]
    with pytest.raises(C.CheckpointError, match="postnet"):
        C.select_vars(names, ["encoder/.*", "postnet/.*"])


def test_warm_start_reads_only_matching_vars(tmp_path, state):
    hp, sl, ent, arena = state
    path = _save(tmp_path, state)
    got = C.load_warm_start(path, sl, ["decoder/prenet.*"])
    assert sorted(got) == sorted(n for n in sl.layout.shapes if n.startswith("decoder/prenet"))
    for k, v in got.items():
        assert v.tobytes() == ent["var/" + k].tobytes()


def test_foreign_files_are_refused(tmp_path, state):
    sl = state[1]
    other = tmp_path / "model.ckpt-7.npz"
    np.savez(other, weights=np.zeros(4, np.float32))
    with pytest.raises(C.CheckpointError, match="not a sat_amd.checkpoint file"):
        C.load(str(other), sl)
    assert C.latest_checkpoint(str(tmp_path)) is None
    meta = np.frombuffer(json.dumps({"format": "something else"}).encode(), np.uint8)
    np.savez(other, meta=meta)
    with pytest.raises(C.CheckpointError, match="not a sat_amd.checkpoint file"):
        C.read_meta(str(other))
    text = tmp_path / "notes.npz"
    text.write_text("not a zip at all")
    with pytest.raises(C.CheckpointError):
        C.load(str(text), sl)
    with pytest.raises(C.CheckpointError):
        C.load(str(tmp_path / "absent.npz"), sl)
    # a TensorFlow checkpoint prefix (model.ckpt-100.index / .data-*) says what it is
    (tmp_path / "model.ckpt-100.index").write_bytes(b"\0")
    (tmp_path / "model.ckpt-100.data-00000-of-00001").write_bytes(b"\0")
    for p in ("model.ckpt-100", "model.ckpt-100.index", "model.ckpt-100.data-00000-of-00001"):
        with pytest.raises(C.CheckpointError, match="TF checkpoint"):
            C.load(str(tmp_path / p), sl)


def test_binding_declares_the_digest_entry():
    from sat_amd import _lib
    assert "sat_arena_digest" in _lib.header_symbols()
    assert len(_lib.SIGNATURES["sat_arena_digest"]) == 6
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        # argument checks come before any device work
        assert lib.sat_arena_digest(None, -1, 0, 0, None, None) != 0
        assert b"sat_arena_digest" in lib.sat_last_error_string()
