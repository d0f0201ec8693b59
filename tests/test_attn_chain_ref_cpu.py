"""Anchors tests/attn_chain_ref.py (the float64 reference of test_attn_chain_gpu.py) to the
oracle's decoder: oracle.decoder_loop on the model's own parameters against attn_chain_ref.chain
fed the operands decoder.py forms (hoisted X0, masked values, keys, the initial alignment state).
CPU only, float64, one small shape."""
import numpy as np
import pytest
import torch

import attn_chain_ref as C

F64 = torch.float64
TOL = 1e-12


def _setup(masked):
    from sat_amd import data, hparams, params
    from oracle import sat_oracle as O
    hp = hparams.ljspeech_hparams()
    d = params.resolve_dims(hp)
    B, N, Tp = 3, 7, 4
    g = torch.Generator().manual_seed(11 + masked)
    p = O.to_torch(params.init_params(hp, seed=9))
    # the initialiser leaves the location-conv bias and the attention bias at zero: give them
    # values, so that a term dropped from the reference would show
    for k in ("decoder/attention1/location_conv/bias", "decoder/attention1/attention_bias"):
        p[k] = 0.3 * torch.randn(p[k].shape, generator=g, dtype=F64)
    m1 = torch.randn(B, N, d.m1, generator=g, dtype=F64)
    m2 = torch.randn(B, N, d.m2, generator=g, dtype=F64)
    lengths = torch.tensor([N, 1, 4])
    targets = torch.randn(B, Tp * hp.outputs_per_step, hp.num_mels, generator=g, dtype=F64)
    masks = O.to_torch(data.synthetic_masks(hp, B, N, Tp, seed=5)) if masked else None
    return O, params, hp, d, p, m1, m2, lengths, targets, masks


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "eval"])
def test_chain_matches_oracle_decoder(masked):
    """chain == oracle.decoder_loop (float64, 1e-12) with zoneout masks and with the eval blend,
    ragged lengths (one full row, one of length 1): the raw attention-RNN outputs, both contexts
    and both alignment histories; REC0 rows carry [c1 | c2 | zoned-out h0], row 0 as given."""
    O, params, hp, d, p, m1, m2, lengths, targets, masks = _setup(masked)
    B, N, _ = m1.shape
    _, ex = O.decoder_loop(m1, m2, lengths, targets, p, hp, masks, record=True)

    # the operands as decoder.py forms them
    x = O.teacher_inputs(targets, hp.outputs_per_step, hp.n_feed_frame)
    pre = O.decoder_prenets(x, p, hp, masks, None).transpose(0, 1)             # [T', B, p]
    Tp, pw = pre.shape[0], pre.shape[-1]
    A, M1, M2 = d.att_rnn, d.m1, d.m2
    name = "decoder/attention_lstm"
    W0 = torch.from_numpy(params.to_internal(f"{name}/kernel", p[f"{name}/kernel"].numpy()))
    b0 = torch.from_numpy(params.to_internal(f"{name}/bias", p[f"{name}/bias"].numpy()))
    X0 = pre @ W0[:pw] + b0
    W0r = W0[pw:pw + M1 + M2 + A]
    mask = O.seq_mask(lengths, N, F64).unsqueeze(-1)
    V1, V2 = m1 * mask, m2 * mask
    a1, a2 = "decoder/attention1", "decoder/attention2"
    mem = (V1 @ p[f"{a1}/memory_layer/kernel"], V1, V2 @ p[f"{a2}/memory_layer/kernel"], V2, lengths)
    par = dict(v1=p[f"{a1}/attention_variable"], b1=p[f"{a1}/attention_bias"],
               convW=p[f"{a1}/location_conv/kernel"].reshape(d.loc_k, d.loc_f),
               convb=p[f"{a1}/location_conv/bias"], locW=p[f"{a1}/location_layer/kernel"],
               v2=p[f"{a2}/attention_v"])
    s0 = torch.zeros(B, N, dtype=F64)
    a0 = torch.zeros(B, N, dtype=F64)
    a0[:, 0] = 1.0                                                    # decoder.py: AL1 row 0
    rec0, c0 = torch.zeros(B, M1 + M2 + A, dtype=F64), torch.zeros(B, A, dtype=F64)
    zm = None if masks is None else (masks["dec/lstm0/zc"], masks["dec/lstm0/zh"])
    o = C.chain(X0, W0r, p[f"{a1}/query_layer/kernel"], p[f"{a2}/query_layer/kernel"], mem, s0, a0,
                rec0, c0, par, zm, hp.zoneout_factor_cell, hp.zoneout_factor_output)

    def close(got, ref, what):
        err = float((got - ref).abs().max())
        assert err <= TOL, (what, err)

    close(o.H0RAW, ex["h0"].transpose(0, 1), "h0'")
    close(o.REC0[1:, :, :M1], ex["c1"].transpose(0, 1), "c1")
    close(o.REC0[1:, :, M1:M1 + M2], ex["c2"].transpose(0, 1), "c2")
    close(o.AL1[1:], ex["alignment1"].transpose(0, 1), "alignment1")
    close(o.S2, ex["alignment2"].transpose(0, 1), "alignment2")
    assert torch.equal(o.REC0[0], rec0) and torch.equal(o.AL1[0], a0) and torch.equal(o.S1[0], s0)
    # shapes of every history, as include/sat_abi.h lays them out
    D = d.d1 + d.d2
    want = dict(REC0=(Tp + 1, B, M1 + M2 + A), C0=(Tp + 1, B, A), H0RAW=(Tp, B, A), G0=(Tp, B, 4 * A),
                Q=(Tp, B, D), S1=(Tp + 1, B, N), AL1=(Tp + 1, B, N), S2=(Tp, B, N), ST=(Tp, B, 4),
                LOC=(Tp, B, N, d.loc_f), ZH=(Tp, B, N, D))
    for k, shp in want.items():
        assert tuple(getattr(o, k).shape) == shp, k
    # past the length: exact zeros in all three alignment histories; each row sums to one
    past = torch.arange(N).unsqueeze(0) >= lengths.unsqueeze(1)
    for h in (o.S1[1:], o.AL1[1:], o.S2):
        assert float(h[:, past].abs().max()) == 0.0
        close(h.sum(-1), torch.ones(Tp, B, dtype=F64), "row sums")
    # ZH is the tanh whose v-weighted sum is the energy, and ST's columns are what they say
    e1 = (o.ZH[..., :d.d1] * par["v1"]).sum(-1).masked_fill(past, float("-inf"))
    close(torch.softmax(e1, -1), o.S1[1:], "softmax(v1 . ZH)")
    close(o.ST[..., 0], e1.max(-1).values, "ST max")
    close(o.ST[..., 1], torch.exp(e1 - o.ST[..., :1]).sum(-1), "ST sum")


def test_chain_grads_match_whole_graph_autograd():
    """chain_grads' intermediate gradients are consistent with one another: DG0 at step t is the
    LSTM's reverse step fed DH0, DQP through the query layers, and the FULL dL/dctx of step t
    through step t+1's context rows -- checked as dL/dX0 == finite differences of the loss in one
    coordinate, and DCTX[T'-1] == RD_in[T'-1] (nothing flows in from beyond the last step)."""
    g = torch.Generator().manual_seed(2)
    r = lambda *s, scale=1.0: scale * torch.randn(*s, generator=g, dtype=F64)   # noqa: E731
    T, B, N, U, M1, M2, D1, D2, F, KW = 3, 2, 6, 4, 5, 3, 6, 2, 2, 4
    mem = (r(B, N, D1), r(B, N, M1), r(B, N, D2), r(B, N, M2), torch.tensor([N, 3]))
    par = dict(v1=r(D1), b1=r(D1), convW=r(KW, F), convb=r(F), locW=r(F, D1), v2=r(D2))
    X0, W0r = r(T, B, 4 * U), r(M1 + M2 + U, U, 4, scale=0.3)
    Wq1, Wq2 = r(U, D1), r(U, D2)
    s0 = torch.softmax(r(B, N), -1)
    a0 = torch.softmax(r(B, N), -1)
    rec0, c0 = r(B, M1 + M2 + U, scale=0.5), r(B, U, scale=0.5)
    DH0, RD = r(T, B, U), r(T, B, M1 + M2)
    args = (W0r, Wq1, Wq2, mem, s0, a0, rec0, c0, par, None, 0.1, 0.2)
    _, gr = C.chain_grads(X0, *args, DH0, RD)
    assert torch.equal(gr["DCTX"][T - 1], RD[T - 1])

    def loss(x):
        o = C.chain(x, *args)
        return float((o.H0RAW * DH0).sum() + (torch.stack(o.ctx) * RD).sum())

    for idx in ((0, 1, 5), (1, 0, 2), (2, 1, 15)):
        h = 1e-6
        xp, xm = X0.clone(), X0.clone()
        xp[idx] += h
        xm[idx] -= h
        fd = (loss(xp) - loss(xm)) / (2 * h)
        assert abs(fd - float(gr["DG0"][idx])) <= 1e-7 * max(1.0, abs(fd)), (idx, fd)
    # the initial rows are read: another initial state gives another step 0
    o1 = C.chain(X0, *args)
    o2 = C.chain(X0, W0r, Wq1, Wq2, mem, s0, a0, torch.zeros_like(rec0), torch.zeros_like(c0), par,
                 None, 0.1, 0.2)
    assert float((o1.H0RAW[0] - o2.H0RAW[0]).abs().max()) > 1e-3
    assert np.isfinite(loss(X0))
