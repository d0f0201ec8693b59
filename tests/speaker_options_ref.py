"""Literal fp64 form of the fork's three speaker options (models/models.py:64-83), shared by
test_speaker_options_cpu.py and test_speaker_options_gpu.py.

The oracle's ``decoder_loop`` takes the memories and the parameter dict as arguments and sizes
everything from them, so the reference is the reference's own text: build ``[m | tile(s)]`` in
torch and hand the widened memories and the widened (TF row order) kernels to it.  Only
``model_forward`` fixes the speaker handling from hparams, so that piece is restated here.  The
transition agent comes from tests/transition_agent_ref.py (its ``[c1 | pq]`` concatenation reads
the widened context, which gives the TF row order ``[c1 | s | pq]``).

Also the numpy restatements of the three kernels of csrc/speaker.hip.
"""
import numpy as np
import torch

# the fixture of the issue: two attention tiles (the second partial), one utterance inside the
# first tile, T' = 6 with r = 1
B, N, T, LENGTHS = 3, 40, 6, (40, 33, 7)
SPK_DIM, PROJ = 16, 8
# Seeds: parameters from init_params(seed=5); the batch (speaker ids included) from
# synthetic_batch(seed=BATCH_SEED).  With these the projection's fp64 pre-activations
# s_raw Wp + bp of the batch's three speakers have min |pre| = 1.529e-02 (3.757e-02 for the fixed
# speaker 300), far from the ReLU kink (bar 1e-4; test_speaker_options_cpu.py asserts it).
PARAM_SEED = 5
BATCH_SEED = 1
FIXED_SPEAKER = 300

OPTIONS = {
    "projection": dict(speaker_embedding_projection_out_dim=PROJ),
    "to_decoder": dict(speaker_embedd_to_decoder=True),
    "to_decoder_only": dict(speaker_embedd_to_decoder=True, speaker_embedd_to_prenet=False),
    "fixed": dict(speaker_for_synthesis=FIXED_SPEAKER),
    "all": dict(speaker_embedding_projection_out_dim=PROJ, speaker_embedd_to_decoder=True,
                speaker_for_synthesis=FIXED_SPEAKER),
}


def make_hparams(key=None, agent=False, **over):
    from sat_amd import hparams
    kw = dict(outputs_per_step=1, speaker_embedding_dim=SPK_DIM)
    if key is not None:
        kw.update(OPTIONS[key])
    if agent:
        kw.update(use_forward_attention_transition_agent=True)
    kw.update(over)
    return hparams.vctk_hparams(**kw)


def make_batch(hp, seed=BATCH_SEED):
    from sat_amd import data
    b = data.synthetic_batch(hp, B, N=N, T=T, shape="max", seed=seed)
    b["source_length"] = np.asarray(LENGTHS, np.int64)
    for i, n in enumerate(LENGTHS):
        b["source"][i, n:] = 0
    return b


def make_values(hp, seed=PARAM_SEED):
    import transition_agent_ref as R
    return R.fixture_values(hp, seed=seed)


def speaker_vector(p, hp, batch):
    """(s [B, S], projection pre-activations or None) -- models/models.py:64-75."""
    ids = batch["speaker_id"]
    if hp.speaker_for_synthesis > -1:
        ids = torch.full_like(ids, hp.speaker_for_synthesis)
    s = p["speaker_embedding"][ids - hp.speaker_embedding_offset]
    pre = None
    if hp.speaker_embedding_projection_out_dim > -1:
        pre = s @ p["speaker_embedding_projection/kernel"] + p["speaker_embedding_projection/bias"]
        s = torch.relu(pre)
    return s, pre


def model_forward(O, p, bufs, hp, batch, masks, training):
    """O.model_forward with the speaker options (the literal tile + concat of :77-83)."""
    m1, m2, _ = O.encoder(batch["source"], batch["source_length"], p, bufs, hp, masks, training)
    s, pre = speaker_vector(p, hp, batch)
    if hp.speaker_embedd_to_decoder:
        tiled = s.unsqueeze(1).expand(-1, m1.shape[1], -1)
        m1 = torch.cat([m1, tiled], dim=-1)
        m2 = torch.cat([m2, tiled], dim=-1)
    spk = s if hp.speaker_embedd_to_prenet else None
    dout, extra = O.decoder_loop(m1, m2, batch["source_length"], batch["mel"], p, hp, masks, spk)
    mel_r, stop, _ = O.decoder_head(dout, p, hp, masks)
    mel = mel_r.reshape(mel_r.shape[0], -1, hp.num_mels)
    loss, l1, bce = O.losses(mel, stop, batch["mel"], batch["mel_mask"], batch["done"],
                             batch["done_mask"])
    out = {"mel": mel, "stop": stop, "loss": loss, "s": s, "pre": pre}
    out.update(extra)
    return out


# ------------------------------------------------------------------ the kernels, in numpy
def rows_bias_fwd_np(y, bias, lengths=None):
    """y [B, N, C] += bias [B, C] on rows n < lengths[b] (all rows without lengths)."""
    out = y.copy()
    for b in range(y.shape[0]):
        n = y.shape[1] if lengths is None else int(min(max(lengths[b], 0), y.shape[1]))
        out[b, :n] = out[b, :n] + bias[b]
    return out


def rows_bias_bwd_np(dy, lengths=None):
    """[B, C] fp64 sums of dy [B, N, C] over rows n < lengths[b]."""
    out = np.zeros((dy.shape[0], dy.shape[2]), np.float64)
    for b in range(dy.shape[0]):
        n = dy.shape[1] if lengths is None else int(min(max(lengths[b], 0), dy.shape[1]))
        out[b] = dy[b, :n].astype(np.float64).sum(0)
    return out


def ctx_tail_fill_np(ctx, col0, s, t0, t1):
    """ctx [T, B, W]: rows t0..t1-1 get s [B, S] in columns col0..col0+S-1."""
    out = ctx.copy()
    out[t0:t1, :, col0:col0 + s.shape[1]] = s[None]
    return out
