"""Eligibility of the multi-speaker (VCTK) decoder for the one-launch free-running decode, asked
without a GPU on the stand-in of test_infer_dropout_cpu.py (what FreeRunningDecoder._why_not
reads: d, hp, forced, feed, m.device), and the ctypes side of the entry's speaker and dropout
options."""
import ctypes
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


def _vctk(drop=False, **over):
    from sat_amd import hparams
    hp = hparams.vctk_hparams(**over)
    if drop:
        hp.set_hparam("apply_dropout_on_inference", True)
    return hp


@pytest.mark.parametrize("drop", [False, True], ids=["clean", "dropout"])
@pytest.mark.parametrize("shape", [(3, 15, 40), (8, 256, 512)])
def test_vctk_preset_is_eligible(shape, drop):
    hp = _vctk(drop)
    from sat_amd import params
    assert params.resolve_dims(hp).multi_speaker
    assert _why_not(hp, *shape) == ""


@pytest.mark.parametrize("drop", [False, True], ids=["clean", "dropout"])
def test_vctk_keeps_the_existing_reasons(drop):
    hp = _vctk(drop)
    bounds = "B={} (<= 8), N={} (<= 256), T'={} (<= 512)"
    assert _why_not(hp, 9, 15, 40) == bounds.format(9, 15, 40)
    assert _why_not(hp, 3, 257, 40) == bounds.format(3, 257, 40)
    assert _why_not(hp, 3, 15, 513) == bounds.format(3, 15, 513)
    assert _why_not(hp, 3, 15, 40, feed="softmax") == "forced alignments / non-mel feedback"
    assert _why_not(hp, 3, 15, 40, forced=(None, None)) == "forced alignments / non-mel feedback"
    assert _why_not(hp, 3, 15, 40, device="cpu") == "not a GPU model"
    assert _why_not(_vctk(drop, speaker_embedd_to_decoder=True), 3, 15, 40) == \
        "speaker_embedd_to_decoder is on the per-step path only"
    assert _why_not(_vctk(drop, use_forward_attention_transition_agent=True), 3, 15, 40) == \
        ("use_forward_attention_transition_agent / cumulative_weights are on the per-step path "
         "only")


def test_options_that_only_change_the_row_are_eligible():
    assert _why_not(_vctk(speaker_embedding_projection_out_dim=8), 3, 15, 40) == ""
    assert _why_not(_vctk(speaker_for_synthesis=300), 3, 15, 40) == ""


def test_other_decoder_dimensions_stay_ineligible():
    """The compiled dimensions still gate: r = 1 names its field."""
    assert _why_not(_vctk(outputs_per_step=1), 3, 15, 40) == "r=1, needs 2"


def test_speaker_struct_matches_the_header():
    """SatDecodeSpeaker: three pointers, laid out as gcc lays out include/sat_abi.h."""
    import test_abi_cpu as A
    from sat_amd import _lib
    st = _lib.SatDecodeSpeaker
    fields = [f for f, _ in st._fields_]
    assert fields == ["spk0", "Wd", "bd"]
    assert ctypes.sizeof(st) == A._c_sizeof("SatDecodeSpeaker")
    assert [getattr(st, f).offset for f in fields] == A._c_offsets("SatDecodeSpeaker", fields)


def test_dropout_struct_matches_the_header():
    """SatDecodeDropout: a pointer, two stream ids and keep, laid out as gcc lays out
    include/sat_abi.h."""
    import test_abi_cpu as A
    from sat_amd import _lib
    st = _lib.SatDecodeDropout
    fields = [f for f, _ in st._fields_]
    assert fields == ["seed", "stream0", "stream1", "keep"]
    assert ctypes.sizeof(st) == A._c_sizeof("SatDecodeDropout")
    assert [getattr(st, f).offset for f in fields] == A._c_offsets("SatDecodeDropout", fields)


def test_entries_check_their_arguments_before_any_device_work():
    """Null speaker rows / a bad keep are refused with the entry's name and the option struct
    at fault in the message."""
    from sat_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsat_hip.so not built")
    lib = _lib.load()
    d, s = _lib.SatDecodePersistent(), _lib.SatDecodeSpeaker()
    dr = _lib.SatDecodeDropout()
    fake = ctypes.c_void_p(16)
    dr.seed, dr.stream0, dr.stream1, dr.keep = fake, 1001, 1002, 0.0
    # a zero shape answers first
    assert lib.sat_decode_persistent(ctypes.byref(d), None, ctypes.byref(s), None, None) != 0
    assert b"sat_decode_persistent: B <= 8" in lib.sat_last_error_string()
    # a valid shape: the null speaker rows answer, before the bad keep and the base struct
    d.B, d.N, d.T = 3, 15, 40
    for drop in (None, ctypes.byref(dr)):
        assert lib.sat_decode_persistent(ctypes.byref(d), drop, ctypes.byref(s), None, None) != 0
        assert b"sat_decode_persistent: spk: null pointer" in lib.sat_last_error_string()
    s.spk0 = s.Wd = s.bd = fake
    rc = lib.sat_decode_persistent(ctypes.byref(d), ctypes.byref(dr), ctypes.byref(s), None, None)
    assert rc != 0
    assert b"sat_decode_persistent: drop:" in lib.sat_last_error_string()
    assert b"keep" in lib.sat_last_error_string()
    dr.keep, dr.seed = 0.5, None
    rc = lib.sat_decode_persistent(ctypes.byref(d), ctypes.byref(dr), ctypes.byref(s), None, None)
    assert rc != 0 and b"sat_decode_persistent: drop: null pointer" in lib.sat_last_error_string()
    # the speaker rows given: the base struct's null-pointer check answers
    assert lib.sat_decode_persistent(ctypes.byref(d), None, ctypes.byref(s), None, None) != 0
    assert b"sat_decode_persistent: null pointer" in lib.sat_last_error_string()
    # and the shape check still comes first (B = 0)
    d.B = 0
    assert lib.sat_decode_persistent(ctypes.byref(d), None, ctypes.byref(s), None, None) != 0
    assert b"B <= 8" in lib.sat_last_error_string()
