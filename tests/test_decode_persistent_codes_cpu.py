"""Eligibility of the VQ-code models (num_mels = num_codes, r = 1) for the one-launch free-running
decode, asked without a GPU on the stand-in of test_decode_persistent_spk_cpu.py; the algebra of
the fed-frame fold FreeRunningDecoder._pack_persistent makes for any output shape, in float64; and
the ctypes side of sat_decode_persistent's option structs (history, speaker, dropout)."""
import ctypes
import os
import types

import pytest
import torch

import _sat_path  # noqa: E402

_sat_path.load()


def _why_not(hp, B, N, Tm, feed="mel", device="cuda", forced=None):
    from sat_amd import params
    from sat_amd.inference import FreeRunningDecoder
    me = types.SimpleNamespace(d=params.resolve_dims(hp), hp=hp, forced=forced, feed=feed,
                               m=types.SimpleNamespace(device=torch.device(device)))
    return FreeRunningDecoder._why_not(me, B, N, Tm)


def _codes(C, multi=False, **over):
    from sat_amd import hparams
    return hparams.codes_hparams(C, **dict(dict(use_speaker_embedding=multi), **over))


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("C", [13, 1025])
def test_cpu_codes_model_is_refused_for_the_device_only(C, multi):
    """The only thing between a codes model and the one-launch decode is the GPU: a CPU model
    gets exactly that reason, not one about num_mels, r or the fed width."""
    from sat_amd import params
    hp = _codes(C, multi)
    d = params.resolve_dims(hp)
    assert (d.num_mels, d.r, d.feed, d.multi_speaker) == (C, 1, C, multi)
    assert _why_not(hp, 3, 15, 40, device="cpu") == "not a GPU model"
    assert _why_not(hp, 3, 15, 40) == ""
    assert _why_not(hp, 8, 256, 512) == ""


def test_codes_models_keep_the_other_reasons():
    hp = _codes(1025, True)
    bounds = "B={} (<= 8), N={} (<= 256), T'={} (<= 512)"
    assert _why_not(hp, 9, 15, 40) == bounds.format(9, 15, 40)
    assert _why_not(hp, 3, 257, 40) == bounds.format(3, 257, 40)
    assert _why_not(hp, 3, 15, 513) == bounds.format(3, 15, 513)
    assert _why_not(hp, 3, 15, 40, feed="softmax") == "forced alignments / non-mel feedback"
    assert _why_not(hp, 3, 15, 40, forced=(None, None)) == "forced alignments / non-mel feedback"
    assert _why_not(_codes(13, n_feed_frame=2, outputs_per_step=2), 3, 15, 40) == \
        "n_feed_frame != 1"
    assert _why_not(_codes(13, True, speaker_embedd_to_decoder=True), 3, 15, 40) == \
        "speaker_embedd_to_decoder is on the per-step path only"
    assert _why_not(_codes(13, attention_out_units=128), 3, 15, 40) == "att_rnn=128, needs 256"


def test_mel_presets_answer_as_before():
    from sat_amd import hparams
    for hp in (hparams.ljspeech_hparams(), hparams.vctk_hparams()):
        assert _why_not(hp, 3, 15, 40) == ""
        assert _why_not(hp, 3, 15, 40, device="cpu") == "not a GPU model"
        assert _why_not(hp, 9, 15, 40) == "B=9 (<= 8), N=15 (<= 256), T'=40 (<= 512)"
        assert _why_not(hp, 3, 15, 40, feed="softmax") == "forced alignments / non-mel feedback"


def test_which_entries_a_model_takes():
    """80 mels x r = 2 keeps the mel-row entries; every other width takes the history ones,
    whatever r is.  An 80-wide model with another r is neither's: it keeps the reason it had."""
    from sat_amd import hparams, params
    from sat_amd.inference import FreeRunningDecoder
    uses = lambda hp: FreeRunningDecoder._uses_history(  # noqa: E731
        types.SimpleNamespace(d=params.resolve_dims(hp)))
    assert not uses(hparams.ljspeech_hparams()) and not uses(hparams.vctk_hparams())
    assert uses(_codes(13)) and uses(_codes(1025, True)) and uses(_codes(81))
    assert _why_not(_codes(7, outputs_per_step=3), 3, 15, 40) == ""
    assert _why_not(hparams.vctk_hparams(outputs_per_step=1), 3, 15, 40) == "r=1, needs 2"
    assert _why_not(_codes(80), 3, 15, 40) == "r=1, needs 2"


# ------------------------------------------------------------------ the fold, in float64
def _gemm64(A, B, C=None, *, bias=None, **kw):
    """K.gemm's contract on host tensors: C = A @ B + bias."""
    assert not kw, kw
    y = A @ B
    if bias is not None:
        y = y + bias
    if C is None:
        return y
    C.copy_(y)
    return C


def _packed(hp, monkeypatch, seed):
    """FreeRunningDecoder._pack_persistent itself, run on float64 host tensors (K.gemm stood in
    by a float64 matmul) with random weights and biases; returns (P, d, pk)."""
    from sat_amd import inference as I
    from sat_amd import params
    d = params.resolve_dims(hp)
    g = torch.Generator().manual_seed(seed)
    P = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) / 8.0
         for k, v in params.init_params(hp, seed=5).items() if k.startswith("decoder/")}
    Mr = d.num_mels * d.r
    MSW = (Mr + 1 + 3) // 4 * 4
    f64 = dict(dtype=torch.float64)
    pl = types.SimpleNamespace(Wms=torch.zeros(d.dsa, MSW, **f64), bms=torch.zeros(MSW, **f64))
    pl.Wms[:, :Mr] = P["decoder/out_projection/kernel"]            # as _prepare packs them
    pl.bms[:Mr] = P["decoder/out_projection/bias"]
    pl.pk = dict(Wzp=torch.empty(256, 256, **f64), bzp=torch.empty(1, 256, **f64),
                 Wq=torch.empty(256, 256, **f64), Wqku=torch.empty(256, 1024, **f64),
                 bqku=torch.zeros(1024, **f64), bz=torch.empty(1, 256, **f64),
                 tmp=torch.empty(2, 128, 256, **f64), y=torch.empty(1, 256, **f64))
    monkeypatch.setattr(I.K, "gemm", _gemm64)
    me = types.SimpleNamespace(m=types.SimpleNamespace(P=P), d=d, hp=hp)
    I.FreeRunningDecoder._pack_persistent(me, pl)
    return P, d, pl.pk


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("M,r", [(13, 1), (1025, 1), (80, 2), (7, 3)])
def test_fold_algebra_float64(monkeypatch, M, r, multi):
    """relu(x_fed W_p0 + b_p0) with x_fed = (z W_out + b_out)[-feed:] equals relu(z Wzp + bzp)
    for the Wzp / bzp _pack_persistent forms, to 1e-12: r = 1 folds the whole projection (odd
    widths included), r > 1 its last num_mels columns.  Multi-speaker: W_p0 is dense0."""
    from sat_amd import hparams
    hp = hparams.codes_hparams(M, outputs_per_step=r, use_speaker_embedding=multi)
    P, d, pk = _packed(hp, monkeypatch, seed=3 + M + r)
    assert (d.num_mels, d.r, d.feed, d.multi_speaker) == (M, r, M, multi)
    p0 = "decoder/prenet0/dense0" if multi else "decoder/prenet0"
    z = torch.randn(5, 256, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    frame = z @ P["decoder/out_projection/kernel"] + P["decoder/out_projection/bias"]
    assert frame.shape[1] == M * r
    x_fed = frame[:, -d.feed:]
    want = torch.relu(x_fed @ P[f"{p0}/kernel"] + P[f"{p0}/bias"])
    got = torch.relu(z @ pk["Wzp"] + pk["bzp"])
    assert float((got - want).abs().max()) <= 1e-12
    assert float(want.abs().max()) > 0.1              # the comparison is not of zeros


# ------------------------------------------------------------------ the ABI side
def test_history_struct_matches_the_header():
    """SatDecodeHistory: four pointers, laid out as gcc lays out include/sat_abi.h."""
    import test_abi_cpu as A
    from sat_amd import _lib
    st = _lib.SatDecodeHistory
    fields = [f for f, _ in st._fields_]
    assert fields == ["ZH", "STOP", "w_stop", "b_stop"]
    assert ctypes.sizeof(st) == A._c_sizeof("SatDecodeHistory")
    assert [getattr(st, f).offset for f in fields] == A._c_offsets("SatDecodeHistory", fields)


def _combinations(lib, d, dr, s, h, history=(True,)):
    """The entry called with every on / off combination of the dropout and speaker options,
    for each ``history`` setting: {"hist+spk+drop": call, ...}."""
    out = {}
    for hist in history:
        for spk in (False, True):
            for drop in (False, True):
                name = "+".join(n for n, on in (("hist", hist), ("spk", spk), ("drop", drop))
                                if on) or "plain"
                out[name] = lambda hist=hist, spk=spk, drop=drop: lib.sat_decode_persistent(
                    ctypes.byref(d), ctypes.byref(dr) if drop else None,
                    ctypes.byref(s) if spk else None, ctypes.byref(h) if hist else None, None)
    return out


def _options(_lib, fake, keep=0.5):
    d, dr = _lib.SatDecodePersistent(), _lib.SatDecodeDropout()
    s, h = _lib.SatDecodeSpeaker(), _lib.SatDecodeHistory()
    dr.seed, dr.stream0, dr.stream1, dr.keep = fake, 1001, 1002, keep
    s.spk0 = s.Wd = s.bd = fake
    h.ZH = h.STOP = h.w_stop = h.b_stop = fake
    return d, dr, s, h


def test_history_entries_check_their_arguments_before_any_device_work():
    """Shapes outside B <= 8, N <= 256, T <= 512, a null or misaligned ZH and a bad keep are
    refused with SAT_ERR_ARGUMENT, the entry's name and the option struct at fault; no device is
    touched (none is here)."""
    from sat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsat_hip.so not built")
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    d, dr, s, h = _options(_lib, fake)
    for B, N, T in ((9, 15, 40), (3, 257, 40), (3, 15, 513), (0, 15, 40)):
        d.B, d.N, d.T = B, N, T
        for name, call in _combinations(lib, d, dr, s, h).items():
            assert call() == _lib.SAT_ERR_ARGUMENT, (name, B, N, T)
            msg = lib.sat_last_error_string()
            assert b"sat_decode_persistent: B <= 8" in msg
            assert f"B={B} N={N} T={T}".encode() in msg
    d.B, d.N, d.T = 3, 15, 40
    for bad in (None, ctypes.c_void_p(20)):                  # null, then not 16-byte aligned
        h.ZH = bad
        for name, call in _combinations(lib, d, dr, s, h).items():
            assert call() == _lib.SAT_ERR_ARGUMENT, name
            assert b"sat_decode_persistent: hist:" in lib.sat_last_error_string()
    h.ZH = fake
    dr.keep = 0.0
    for name, call in _combinations(lib, d, dr, s, h).items():
        if name.endswith("drop"):
            assert call() == _lib.SAT_ERR_ARGUMENT
            msg = lib.sat_last_error_string()
            assert b"sat_decode_persistent: drop:" in msg and b"keep" in msg
    # everything of the option structs given: the check of the base struct answers
    dr.keep = 0.5
    for name, call in _combinations(lib, d, dr, s, h).items():
        assert call() == _lib.SAT_ERR_ARGUMENT, name
        assert b"sat_decode_persistent: null pointer" in lib.sat_last_error_string()


def test_every_combination_refuses_a_bad_shape_alike():
    """All eight combinations of the three options answer an out-of-range shape with the same
    message, whatever else is wrong with the options: the shape check comes first."""
    from sat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsat_hip.so not built")
    lib = _lib.load()
    d, dr, s, h = _options(_lib, None, keep=0.0)        # null option pointers, keep = 0
    for B, N, T in ((9, 15, 40), (3, 257, 40), (3, 15, 513), (0, 15, 40)):
        d.B, d.N, d.T = B, N, T
        msgs = set()
        calls = _combinations(lib, d, dr, s, h, history=(False, True))
        assert len(calls) == 8
        for name, call in calls.items():
            assert call() == _lib.SAT_ERR_ARGUMENT, (name, B, N, T)
            msgs.add(lib.sat_last_error_string())
        assert len(msgs) == 1, msgs
        msg = msgs.pop()
        assert msg.startswith(b"sat_decode_persistent: B <= 8, N <= 256, T <= 512")
        assert f"B={B} N={N} T={T}".encode() in msg
