"""Checkpoints on the GPU: ``sat_arena_digest`` against its numpy restatement (exact), bitwise
resume through ``model_dir``, restore under live captured steps, PREDICT / EVAL after a restore,
warm start, the non-finite guard and the one-rank RCCL digest exchange.

All equalities are bitwise.  Shapes: LJSpeech hparams at B=2, N=13, T=16 (the smoke shape), four
fixed synthetic batches of one padded shape."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


# ------------------------------------------------------------------ the digest kernel
def _random_words(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n:                                     # planted inf / NaN / denormal words
        for k, bits in enumerate((0x7F800000, 0xFF800000, 0x7FC00001, 0x00000001)):
            w[(k * 7919) % n] = bits
    return w


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1021, 4099, 1_000_003])
def test_digest_kernel_matches_host(cuda, n):
    from sat_amd import checkpoint as C
    w = _random_words(n, seed=n)
    # a 16-byte-aligned base and one offset by a word from the boundary
    buf = torch.zeros(n + 8, dtype=torch.int32, device=cuda)
    for shift in (0, 1):
        base = (-(buf.data_ptr() // 4) % 4) + shift
        dst = buf[base:base + n]
        assert n == 0 or dst.data_ptr() % 16 == 4 * shift
        dst.copy_(torch.from_numpy(w.view(np.int32)))
        for base_index in (0, 7, (1 << 33) + 5):
            want = C.digest_host(w, base_index)
            assert C.device_digest(dst, base_index) == want, (n, shift, base_index)
            assert C.device_digest(dst, base_index, count_nonfinite=False) == (want[0], 0)


def test_digest_accumulates_and_chains(cuda):
    from sat_amd import checkpoint as C
    from sat_amd import kernels as K
    w = _random_words(4099, seed=1)
    d = torch.from_numpy(w.view(np.int32)).to(cuda)
    out = torch.empty(4, dtype=torch.int32, device=cuda)
    K.fill_(out, 0)
    C.device_digest(d[:1000], 0, True, out=out)          # two calls into the same out[]
    C.device_digest(d[1000:], 1000, True, out=out)
    got = out.cpu().numpy().view(np.uint64)
    assert (int(got[0]), int(got[1])) == C.digest_host(w)
    C.device_digest(d, 5, True, out=out)                 # a third accumulates on top
    got = out.cpu().numpy().view(np.uint64)
    a, b = C.digest_host(w), C.digest_host(w, 5)
    assert (int(got[0]), int(got[1])) == ((a[0] + b[0]) & M64, a[1] + b[1])
    # position matters on the device as on the host
    sw = w.copy()
    sw[[10, 4000]] = sw[[4000, 10]]
    assert C.device_digest(torch.from_numpy(sw.view(np.int32)).to(cuda))[0] != a[0]
    # float tensors and int64 tensors are read as their words
    f = torch.tensor([1.0, float("inf"), float("nan"), 1e-45], device=cuda)
    assert C.device_digest(f) == C.digest_host(f.cpu().numpy()) and C.device_digest(f)[1] == 2
    q = torch.tensor([3, -1, 1 << 40], dtype=torch.int64, device=cuda)
    assert C.device_digest(q, 9, False) == (C.digest_host(q.cpu().numpy(), 9)[0], 0)


# ------------------------------------------------------------------ training runs
def _hp():
    from sat_amd import hparams
    return hparams.ljspeech_hparams(max_iters=24)


@pytest.fixture(scope="module")
def batches():
    from sat_amd import models
    it = models.synthetic_input_fn(_hp(), 2, N=13, T=16, shape="ljs", seed=20)()
    out = [next(it) for _ in range(4)]
    assert len({b[0].source.shape for b in out}) == 1
    return out


def _model(cuda, seed=1234, **kw):
    from sat_amd import models
    return models.DualSourceSelfAttentionTacotronModel(_hp(), device=cuda, seed=seed, **kw)


def _feed(bs):
    return lambda: iter(bs)


def _state(m):
    t = m._trainer
    torch.cuda.synchronize()
    return {"params": m.engine.params.cpu(), "exp_avg": t.exp_avg.cpu(),
            "exp_avg_sq": t.exp_avg_sq.cpu(), "bn": m.engine.bn.buf.cpu(),
            "global_step": t.global_step.cpu(), "seed": t.seed.cpu(), "status": t.status.cpu()}


def _same(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.fixture(scope="module")
def runs(cuda, batches, tmp_path_factory):
    """A: four uninterrupted steps (twice: the precondition).  B: two steps, then a save."""
    a = _model(cuda)
    a.train(_feed(batches), 4)
    a2 = _model(cuda)
    a2.train(_feed(batches), 4)
    b = _model(cuda)
    b.train(_feed(batches[:2]), 2)
    d = tmp_path_factory.mktemp("ckpt_b")
    path = b._trainer.save(str(d / "model.ckpt-2.npz"))
    return {"A": _state(a), "A2": _state(a2), "B": _state(b), "b": b, "dir": str(d),
            "path": path}


def test_uninterrupted_runs_agree(runs):
    assert _same(runs["A"], runs["A2"]) == []
    assert int(runs["A"]["global_step"]) == 4 and int(runs["B"]["global_step"]) == 2
    assert int(runs["A"]["status"][0]) == 0


def test_bitwise_resume_through_model_dir(cuda, batches, runs, tmp_path):
    import shutil
    from sat_amd import checkpoint as C
    from sat_amd import models
    assert os.path.basename(runs["path"]) == "model.ckpt-2.npz"
    assert C.latest_checkpoint(runs["dir"]) == runs["path"]
    d = str(tmp_path)                              # C's own model_dir, holding B's file
    shutil.copy(runs["path"], d)
    c = models.DualSourceSelfAttentionTacotronModel(_hp(), model_dir=d, device=cuda, seed=77)
    assert c._trainer is None and c._pending is not None      # optimiser state still pending
    assert torch.equal(c.engine.params.cpu(), runs["B"]["params"])
    assert torch.equal(c.engine.bn.buf.cpu(), runs["B"]["bn"])
    c.train(_feed(batches[2:]), 2)                 # steps 3 and 4
    assert _same(_state(c), runs["A"]) == []
    assert [s for s, _ in C.list_checkpoints(d)] == [2, 4]


def test_restore_under_live_graphs(cuda, batches, runs):
    g = _model(cuda, seed=5, graph_cache=2)
    g.train(_feed(batches[:2]), 2)                 # first sighting eager + capture, then a replay
    assert g._graphs.misses == 1 and g._graphs.hits == 1
    t = g._trainer
    arenas = (g.engine.params, t.exp_avg, t.exp_avg_sq, g.engine.bn.buf, t.global_step, t.seed,
              t.status, g.engine.exchange)
    ptrs = [x.data_ptr() for x in arenas]
    assert _same(_state(g), runs["B"]) != []       # another init seed: another state
    g.restore(runs["path"])
    assert _same(_state(g), runs["B"]) == []
    g.train(_feed(batches[2:]), 2)                 # two replays of the graph captured before
    assert g._graphs.misses == 1 and g._graphs.hits == 3
    assert _same(_state(g), runs["A"]) == []
    assert [x.data_ptr() for x in arenas] == ptrs


def test_construction_resumes_and_train_saves(cuda, batches, runs, tmp_path):
    """model_dir drives everything: a snapshot every save_checkpoints_steps and at the end,
    keep_checkpoint_max honoured, a new model resumes at the newest file's step."""
    from sat_amd import checkpoint as C
    from sat_amd import models
    hp = _hp()
    hp.save_checkpoints_steps = 1
    hp.keep_checkpoint_max = 2
    d = str(tmp_path / "run")
    m = models.DualSourceSelfAttentionTacotronModel(hp, model_dir=d, device=cuda)
    m.train(_feed(batches), 3)
    assert [s for s, _ in C.list_checkpoints(d)] == [2, 3]
    hp.save_checkpoints_steps = 50
    r = models.DualSourceSelfAttentionTacotronModel(hp, model_dir=d, device=cuda, seed=9)
    assert r._host_step == 3
    r.train(_feed(batches[3:]), 1)                 # step 4: the end-of-train snapshot
    assert int(r._trainer.global_step.item()) == 4
    assert _same(_state(r), runs["A"]) == []
    assert [s for s, _ in C.list_checkpoints(d)] == [3, 4]
    ent, meta = C.read_entries(C.latest_checkpoint(d))
    assert meta["global_step"] == 4 and int(ent["global_step"][0]) == 4
    assert ent["var/embedding"].tobytes() == \
        r.engine.params_dict()["embedding"].tobytes()


def test_predict_after_load_equals_the_saver(cuda, batches, runs):
    from sat_amd import models
    b = runs["b"]
    feats = [(batches[0][0], None)]
    want = next(b.predict(_feed(feats)))
    fresh = _model(cuda, seed=3)
    got = next(fresh.predict(_feed(feats), checkpoint_path=runs["path"]))
    assert fresh._trainer is None
    for k in ("mel", "stop_token", "alignment", "alignment2", "codes"):
        assert torch.equal(want[k], got[k]), k
    # with no name: the newest file of model_dir
    hp = _hp()
    named = models.DualSourceSelfAttentionTacotronModel(hp, model_dir=runs["dir"], device=cuda,
                                                        seed=4)
    again = next(named.predict(_feed(feats)))
    assert torch.equal(want["mel"], again["mel"])


def test_eval_after_restore_uses_the_restored_weights(cuda, batches, runs):
    b = runs["b"]
    want = b.evaluate(_feed(batches[3:]), 1)["loss"]
    m = _model(cuda, seed=6)
    before = m.evaluate(_feed(batches[3:]), 1)["loss"]       # builds the cached eval decoder
    assert m._eval_decoder is not None
    after = m.evaluate(_feed(batches[3:]), 1, checkpoint_path=runs["path"])["loss"]
    assert after == want and before != want


def test_warm_start_takes_only_the_matching_variables(cuda, runs):
    from sat_amd import checkpoint as C
    from sat_amd import models, params
    hp = _hp()
    ws = models.WarmStartSettings(runs["path"], ["encoder/.*"])
    m = models.DualSourceSelfAttentionTacotronModel(hp, device=cuda, seed=11, warm_start_from=ws)
    own = params.init_params(hp, seed=11)
    ent, _ = C.read_entries(runs["path"], prefixes=("var/",))
    got = m.engine.params_dict()
    n_enc = 0
    for k, v in got.items():
        src = ent["var/" + k] if k.startswith("encoder/") else own[k]
        n_enc += k.startswith("encoder/")
        assert v.tobytes() == src.tobytes(), k
    assert n_enc > 20 and m._pending is None and m._host_step == 0
    assert torch.equal(m.engine.bn.buf.cpu(), _model(cuda, seed=11).engine.bn.buf.cpu())
    # a path alone warm-starts every variable; moments stay zero and the step 0
    m2 = models.DualSourceSelfAttentionTacotronModel(hp, device=cuda, seed=12,
                                                     warm_start_from=runs["path"])
    assert torch.equal(m2.engine.params.cpu(), runs["B"]["params"])
    t = m2._get_trainer({"source": torch.zeros(2, 13), "mel": torch.zeros(2, 16, 80)})
    assert int(t.global_step.item()) == 0
    assert not bool(t.exp_avg.any()) and not bool(t.exp_avg_sq.any())
    with pytest.raises(C.CheckpointError, match="postnet"):
        models.DualSourceSelfAttentionTacotronModel(
            hp, device=cuda, warm_start_from=models.WarmStartSettings(runs["path"],
                                                                      ["postnet/.*"]))


def test_failed_restore_leaves_the_model_untouched(cuda, runs, tmp_path):
    from sat_amd import checkpoint as C
    m = _model(cuda, seed=13)
    before = m.engine.params.clone()
    ent, meta = C.read_entries(runs["path"])
    del ent["adam_m/embedding"]
    bad = C.write_entries(str(tmp_path / "bad.npz"), ent, meta)
    with pytest.raises(C.CheckpointError, match="adam_m/embedding"):
        m.restore(bad)
    # a file whose content no longer matches its stored digest is caught on the device
    ent, meta = C.read_entries(runs["path"])
    ent["var/embedding"] = ent["var/embedding"].copy()
    ent["var/embedding"][0, 0] += 1.0
    bad = C.write_entries(str(tmp_path / "flipped.npz"), ent, meta)
    with pytest.raises(C.CheckpointError, match="digest after upload"):
        m.restore(bad)
    assert torch.equal(before, m.engine.params) and m._pending is None


def test_nonfinite_state_is_never_written(cuda, batches, tmp_path):
    from sat_amd import checkpoint as C
    m = _model(cuda)
    m.train(_feed(batches[:1]), 1)
    t = m._trainer
    d = tmp_path / "nan"
    d.mkdir()
    m.engine.params[12345] = float("nan")
    t.snapshot(str(d))
    with pytest.raises(C.CheckpointError, match="non-finite"):
        t.wait()
    t.snapshot(str(d))                         # the error also surfaces from the next snapshot
    with pytest.raises(C.CheckpointError, match="non-finite"):
        t.snapshot(str(d))
    assert t.wait() is None and os.listdir(d) == []
    # a skipped step (status[0] != 0) is refused the same way
    m.engine.params[12345] = 0.0
    t.status[0] = 1
    with pytest.raises(C.CheckpointError, match="skipped"):
        t.save(str(d / "model.ckpt-1.npz"))
    assert os.listdir(d) == []


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_one_rank_group_digest_exchange(cuda, batches, runs, tmp_path):
    """A one-rank nccl group: the forced all-gather of the digest passes and rank 0's file is
    the file of a save made without a process group, array for array."""
    import torch.distributed as tdist
    from sat_amd import checkpoint as C
    assert not tdist.is_initialized(), "an earlier test left a process group open"
    tdist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0,
                             world_size=1, device_id=cuda)
    try:
        m = _model(cuda)
        m.train(_feed(batches[:2]), 2)
        t = m._trainer
        p = str(tmp_path / "model.ckpt-2.npz")
        t.snapshot(path=p, force_exchange=True)
        assert t.wait() == p
        assert t._snapshotter._gath is not None and t._snapshotter._gath.numel() == 3
        g = t._snapshotter._gath_host.numpy().view(np.uint64)
        sl = t._snapshotter.sl
        ck = C.load(p, sl)
        assert (int(g[0]), int(g[1])) == C.digest_host(ck.arena.view(np.uint32)[:sl.n_f])
        assert int(g[2]) == 0                           # no rank carried an error flag
    finally:
        tdist.destroy_process_group()
    with np.load(p) as z1, np.load(runs["path"]) as z2:
        assert sorted(z1.files) == sorted(z2.files)
        for k in z1.files:
            assert z1[k].tobytes() == z2[k].tobytes(), k
