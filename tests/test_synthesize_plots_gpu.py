"""``write_predictions(plots=True, records=True)`` on the GPU: a tiny random-weight LJSpeech-shaped
model decodes three utterances (N = 9..15, max_iters = 12); the plot files must decode to the
canvases tests/figure_ref.py composes from the same predictions copied to the host, the records
must carry the mel files' bytes, and the files written with the switches off must be those of a
call without this feature's arguments.

The same through ``predict_codes(plots=True)`` on the tests/golden/codes fixtures (two utterances,
batch size 1, max_iters = 24, a random-weight model: seconds)."""
import os

import numpy as np
import pytest
import torch

import figure_ref as R

pytestmark = pytest.mark.gpu

GEO = dict(Hp=12, Wp=40, margin=2, cbar=3)
KEYS = ["utt-a", "utt-b", "utt-c"]


@pytest.fixture(scope="module")
def predicted(cuda):
    from sat_amd import data, datasets, hparams, models as MD, params
    hp = hparams.ljspeech_hparams()
    hp.set_hparam("max_iters", 12)
    model = MD.DualSourceSelfAttentionTacotronModel(hp, device=cuda,
                                                    init_values=params.init_params(hp, seed=5))
    b = data.synthetic_batch(hp, 3, N=15, T=16, shape="ljs", seed=6)
    b["source_length"][:] = [15, 12, 9]
    feats = datasets.SourceDataForPrediction(
        id=np.array([11, 12, 13]), key=np.array(KEYS, dtype=object), source=b["source"],
        source_length=b["source_length"],
        text=np.array([b"first text", b"second", b"third"], dtype=object), mel=b["mel"],
        mel_width=np.full(3, hp.num_mels), target_length=np.array([16, 12, 14]))
    p = model.model_fn(feats, None, MD.ModeKeys.PREDICT, hp).predictions
    torch.cuda.synchronize()
    return hp, p


def test_plots_and_records_beside_the_mel_files(predicted, tmp_path):
    from sat_amd import plots, synthesize as S, tfrecord as T
    hp, p = predicted
    ext = hp.predicted_mel_extension
    plain, off, on = (str(tmp_path / d) for d in ("plain", "off", "on"))
    S.write_predictions([p], plain, hp, wav=False)
    S.write_predictions([p], off, hp, wav=False, plots=False, records=False)
    keys = S.write_predictions([p], on, hp, wav=False, plots=True, records=True, plot_options=GEO)
    assert keys == KEYS
    assert sorted(os.listdir(plain)) == sorted(os.listdir(off)) == [f"{k}.{ext}" for k in KEYS]
    assert sorted(os.listdir(on)) == sorted(f"{k}.{e}" for k in KEYS
                                            for e in (ext, "png", "tfrecord"))
    read = lambda d, name: open(os.path.join(d, name), "rb").read()          # noqa: E731
    for k in KEYS:
        assert read(plain, f"{k}.{ext}") == read(off, f"{k}.{ext}") == read(on, f"{k}.{ext}")

    # the reference canvases, from the predictions copied to the host
    host = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in p.items()}
    r, M = int(hp.outputs_per_step), int(hp.num_mels)
    frames = S.stop_frames(host["stop_token"], r, host["mel"].shape[1])
    steps = [f // r for f in frames]
    panels = plots.prediction_panels(host, hp, frames)
    n_heads = sum(1 for name in ("alignment3", "alignment4") if name in p)
    assert n_heads >= 1 and len(panels[0]) == 2 + n_heads + 2
    for b in range(3):
        crops = [(q.rows, q.cols) for q in panels[b]]
        assert crops == ([(int(host["source_length"][b]), steps[b])] * 2
                         + [(steps[b], steps[b])] * n_heads
                         + [(M, int(host["ground_truth_mel_length"][b])), (M, frames[b])])
    # the crops address what they should: panel 0 of utterance 1 is alignment[1, :n, :steps]
    q = panels[1][0]
    flat = np.asarray(q.src).reshape(-1)
    crop = flat[q.base + np.arange(q.cols)[None, :] * q.col_stride + np.arange(q.rows)[:, None]]
    assert (crop == host["alignment"][1, :q.rows, :q.cols]).all()
    want = R.render(panels, plots.default_tables(), GEO["Hp"], GEO["Wp"], GEO["margin"],
                    GEO["cbar"])
    texts = ["first text", "second", "third"]
    for b, k in enumerate(KEYS):
        pixels, text = R.decode_png(read(on, f"{k}.png"))
        assert pixels.shape == want[b].shape == (
            len(panels[0]) * 12 + (len(panels[0]) + 1) * 2, 40 + 3 + 6, 3)
        differ = int((pixels != want[b]).sum())
        print(f"{k}: bytes that differ {differ} of {pixels.size}")
        assert differ == 0
        assert text == {"key": k, "text": texts[b]}
        rec = T.parse_prediction_result(next(T.read_tfrecords(os.path.join(on, f"{k}.tfrecord"))))
        assert rec.codes.tobytes() == read(on, f"{k}.{ext}")
        assert (rec.codes_length, rec.codes_width) == (frames[b], M)
        assert (rec.id, rec.key, rec.text) == (11 + b, k.encode(), texts[b].encode())
        n = int(host["source_length"][b])
        assert rec.source_length == n and rec.source.tolist() == host["source"][b, :n].tolist()
        t = int(host["ground_truth_mel_length"][b])
        assert rec.ground_truth_codes.tobytes() == \
            np.ascontiguousarray(host["ground_truth_mel"][b, :t], "<f4").tobytes()


# ---------------------------------------------------------------- predict_code --plots
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codes")
C_MODEL = 16


def test_predict_code_plots(cuda, tmp_path):
    """The code corpus: the files of a run without ``plots`` are unchanged by it, and each
    ``<key>.png`` equals the reference on the same predictions -- alignments, self-attention
    heads, the true one-hot frames (the target's own length) and the predicted one-hot frames."""
    from sat_amd import datasets as D, hparams, kernels as K, models as MD, params, plots
    from sat_amd import predict_code as PC, preprocess, tfrecord as T
    from sat_amd.synthesize import stop_frames
    hp = hparams.codes_hparams(C_MODEL, source="char", phoneme="none", max_iters=24)
    records = tmp_path / "records"
    preprocess.Codes(GOLDEN, str(records), hp, C_MODEL, compact=True).run()
    keys = ["p225_001", "p225_test"]
    model = MD.DualSourceSelfAttentionTacotronModel(hp, device=cuda,
                                                    init_values=params.init_params(hp, seed=5))

    def input_fn():
        ds = D.create_from_tfrecord_files([str(records / f"{k}.source.tfrecord") for k in keys],
                                          [str(records / f"{k}.target.tfrecord") for k in keys],
                                          hp, cycle_length=1)
        return iter(ds.prepare_and_zip().group_by_batch(1).merge_target_to_source().dataset)

    off, on = tmp_path / "off", tmp_path / "on"
    assert PC.predict_codes(model, input_fn, str(off), hp) == keys
    assert PC.predict_codes(model, input_fn, str(on), hp, plots=True, plot_options=GEO) == keys
    names = sorted(os.listdir(off))
    assert sorted(os.listdir(on)) == sorted(names + [f"{k}.png" for k in keys])
    for name in names:
        assert (on / name).read_bytes() == (off / name).read_bytes()
    for p, (features, _) in zip(model.predict(input_fn), input_fn()):
        key = features.key[0].decode()
        frames = stop_frames(p["stop_token"], 1, p["mel"].shape[1])
        onehot = K.codes_argmax(p["mel"].contiguous(), onehot=True)[1].cpu().numpy()
        truth = T.index_to_one_hot(features.code_index, C_MODEL)[None]
        host = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else v)
                for k, v in p.items()}
        host.update(source_length=features.source_length, ground_truth_mel=truth,
                    ground_truth_mel_length=np.array([truth.shape[1]]))
        panels = plots.prediction_panels(host, hp, frames, mel=onehot)
        assert (panels[0][-2].rows, panels[0][-2].cols) == (C_MODEL, len(features.code_index))
        assert (panels[0][-1].rows, panels[0][-1].cols) == (C_MODEL, frames[0])
        want = R.render(panels, plots.default_tables(), GEO["Hp"], GEO["Wp"], GEO["margin"],
                        GEO["cbar"])
        pixels, text = R.decode_png((on / f"{key}.png").read_bytes())
        assert (pixels == want[0]).all()
        assert text["key"] == key and text["text"] == (on / f"{key}.txt").read_text()
