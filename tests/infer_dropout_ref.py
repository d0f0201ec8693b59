"""Free-running decode with prenet dropout kept on (apply_dropout_on_inference), restated from
the oracle's own building blocks.

``oracle.sat_oracle.infer_free_running`` takes no masks, so its loop (stop-token and validation
helpers, mel / softmax / target feedback) is restated here around ``O.prenet``, which does: the
one added argument is ``masks = (mask0, mask1)``, the step-major ``[T'][B][P_l]`` mask of each
decoder prenet layer, ``None`` for a layer that stays clean.  With ``(None, None)`` the result
equals ``O.infer_free_running`` exactly (test_infer_dropout_cpu.py).  The arithmetic follows the
dtype of the parameters: float64 is the reference, float32 gives the scale ``e32`` the GPU
comparisons are bounded by.

Also the host restatement of the mask layout: which Philox counter and word element
``(t, b, col)`` of a ``[T'][B][P]`` mask uses.
"""
import numpy as np
import torch

from oracle import sat_oracle as O

import philox_ref


def prenets_masked(x, p, hp, spk, m0, m1):
    """O.decoder_prenets for one step's [B, .] input with explicit per-layer masks [B, P_l]."""
    n = len(hp.decoder_prenet_out_units)
    mk = [m0, m1] + [None] * (n - 2)
    if spk is not None:                       # MultiSpeakerPreNet, multi_speaker_modules.py:27-32
        d0 = O.dense(x, p, "decoder/prenet0/dense0", torch.relu)
        d0 = d0 + O.dense(spk, p, "decoder/prenet0/speaker_projection",
                          torch.nn.functional.softsign)
        y = O.dense(d0, p, "decoder/prenet0/dense", torch.relu)
        y = y * mk[0] if mk[0] is not None else y
        start = 1
    else:
        y, start = x, 0
    for i in range(start, n):
        y = O.prenet(y, p, f"decoder/prenet{i}", mk[i])
    return y


def infer_free_running_masked(p, bufs, hp, batch, masks=(None, None), max_iters=None,
                              min_iters=10, feed="mel", helper=None):
    """O.infer_free_running (oracle/sat_oracle.py:517-594, without forced alignments) with the
    prenet masks of step t = ``masks[l][t]``."""
    max_iters = hp.max_iters if max_iters is None else max_iters
    helper = "stop_token" if helper is None else helper
    tg = None
    if helper == "validation":
        max_iters = batch["mel"].shape[1] // hp.outputs_per_step
    if feed == "target":
        assert helper == "validation"
        tg = batch["mel"].reshape(batch["mel"].shape[0], max_iters, -1)
    m1, m2, enc_al = O.encoder(batch["source"], batch["source_length"], p, bufs, hp, None, False)
    spk = None
    if hp.use_speaker_embedding and hp.speaker_embedd_to_prenet:
        spk = p["speaker_embedding"][batch["speaker_id"] - hp.speaker_embedding_offset]
    lengths = batch["source_length"]
    B, N, _ = m1.shape
    M, r, nf = hp.num_mels, hp.outputs_per_step, hp.n_feed_frame
    att1 = O.make_attention(hp.attention, p, "decoder/attention1", m1, lengths)
    att2 = O.make_attention(hp.attention2, p, "decoder/attention2", m2, lengths)
    dt = m1.dtype
    A, D = hp.attention_out_units, hp.decoder_out_units
    st1 = att1.initial_state(B, N, dt)
    st2 = att2.initial_state(B, N, dt)
    c1 = m1.new_zeros(B, m1.shape[2])
    c2 = m2.new_zeros(B, m2.shape[2])
    c0 = h0 = m1.new_zeros(B, A)
    cc1 = hh1 = m1.new_zeros(B, D)
    cc2 = hh2 = m1.new_zeros(B, D)
    zc, zh = hp.zoneout_factor_cell, hp.zoneout_factor_output
    x = m1.new_zeros(B, M * nf)
    hist, mels, stops, al1, al2 = [], [], [], [], []
    probs = None
    for t in range(max_iters):
        pre = prenets_masked(x, p, hp, spk, *(None if m is None else m[t].to(dt) for m in masks))
        cell_in = torch.cat([pre, c1, c2], dim=-1)
        h0_out, c0, h0 = O.zoneout_lstm_step(cell_in, c0, h0, p["decoder/attention_lstm/kernel"],
                                             p["decoder/attention_lstm/bias"], zc, zh, None, None)
        a1, st1 = att1(h0_out, st1)
        a2, st2 = att2(h0_out, st2)
        c1 = (a1.unsqueeze(1) @ att1.values).squeeze(1)
        c2 = (a2.unsqueeze(1) @ att2.values).squeeze(1)
        o = torch.cat([h0_out, c1, c2], dim=-1)
        h1_out, cc1, hh1 = O.zoneout_lstm_step(o, cc1, hh1, p["decoder/lstm1/kernel"],
                                               p["decoder/lstm1/bias"], zc, zh, None, None)
        h2_out, cc2, hh2 = O.zoneout_lstm_step(h1_out, cc2, hh2, p["decoder/lstm2/kernel"],
                                               p["decoder/lstm2/bias"], zc, zh, None, None)
        hist.append(h2_out)
        z = torch.stack(hist, dim=1)
        probs = []
        for h in range(hp.decoder_self_attention_num_hop):
            z, a = O.sa_transformer(z, p, f"decoder/self_attention{h}",
                                    hp.decoder_self_attention_num_heads, True, None)
            probs.append(a)
        last = z[:, -1]
        mel_t = O.dense(last, p, "decoder/out_projection")
        stop_t = O.dense(last, p, "decoder/stop_token_projection")[:, 0]
        mels.append(mel_t)
        stops.append(stop_t)
        al1.append(a1)
        al2.append(a2)
        if feed == "softmax":
            x = torch.softmax(mel_t.view(B, r, M), dim=-1).reshape(B, r * M)[:, -M * nf:]
        elif feed == "target":
            x = tg[:, t, -M * nf:]
        else:
            x = mel_t[:, -M * nf:]
        if helper == "stop_token" and t > min_iters and bool((torch.sigmoid(stop_t) > 0.5).all()):
            break
    T_out = len(mels)
    mel = torch.stack(mels, dim=1).reshape(B, T_out * r, M)
    return {"mel": mel, "stop": torch.stack(stops, dim=1), "alignment1": torch.stack(al1, 1),
            "alignment2": torch.stack(al2, 1), "decoder_self_alignments": probs,
            "encoder_self_alignments": enc_al, "steps": T_out, "m1": m1, "m2": m2}


def mask_element(t, b, col, B, P, seed, stream_id, keep, on):
    """The value of element (t, b, col) of a step-major [T'][B][P] mask, from the layout rule
    alone: index i = (t B + b) P + col, Philox counter {i // 4, stream id}, key = seed, word
    i % 4, on iff float32(word) * 2^-32 < float32(keep)."""
    i = (t * B + b) * P + col
    g = i // 4
    seed, stream_id = int(seed) % (1 << 64), int(stream_id) % (1 << 64)
    r = philox_ref.philox4x32_10(g & 0xFFFFFFFF, g >> 32, stream_id & 0xFFFFFFFF,
                                 stream_id >> 32, seed & 0xFFFFFFFF, seed >> 32)
    w = np.float32(np.uint32(r[i % 4]))
    kept = np.float32(keep) >= np.float32(1.0) or w * np.float32(2.0 ** -32) < np.float32(keep)
    return np.float32(on) if kept else np.float32(0.0)


def host_masks(d, Tm, B, seed, keep, stream0):
    """The masks FreeRunningDecoder draws for a (T', B) decode, from philox_ref: one
    [T'][B][P_l] float32 array per prenet layer, None for a layer that stays clean."""
    from sat_amd.inference import drop_on_value, prenet_drops
    out = []
    for i, drops in enumerate(prenet_drops(d)):
        P = d.dec_prenet[i]
        out.append(philox_ref.mask(Tm * B * P, seed, stream0 + i, keep,
                                   drop_on_value(keep)).reshape(Tm, B, P) if drops else None)
    return out


def as32(d):
    """A dict of float64 oracle tensors in float32 (integer tensors unchanged)."""
    return {k: v.to(torch.float32) if v.is_floating_point() else v for k, v in d.items()}
