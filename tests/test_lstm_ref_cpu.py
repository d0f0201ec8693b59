"""Anchors tests/lstm_ref.py (the kernels'-layout reference of the LSTM GPU tests) to the float64
oracle, and its hand-written reverse step to autograd of its own forward step.  CPU only."""
import numpy as np
import pytest
import torch

import lstm_ref as R

F64 = torch.float64
NAME = "encoder/cbhg/lstm_fw"          # an LSTM-named parameter: to_internal interleaves it


def _rand(g, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=g, dtype=F64)


def _internal(kernel_tf, bias_tf):
    """TF-layout kernel [K][4U] / bias [4U] -> the kernels' [K][U][4] / [U][4]."""
    from sat_amd import params
    K, G = kernel_tf.shape
    Wi = torch.from_numpy(params.to_internal(f"{NAME}/kernel", kernel_tf.numpy())).view(K, G // 4, 4)
    bi = torch.from_numpy(params.to_internal(f"{NAME}/bias", bias_tf.numpy())).view(G // 4, 4)
    # and back: the conversion the tests rely on is a bijection
    assert np.array_equal(params.from_internal(f"{NAME}/kernel", Wi.reshape(K, G).numpy()),
                          kernel_tf.numpy())
    assert np.array_equal(params.from_internal(f"{NAME}/bias", bi.reshape(G).numpy()),
                          bias_tf.numpy())
    return Wi, bi


def _gates_tf(gates):
    """[B][U][4] -> TF column order [B][4U]."""
    from sat_amd import params
    B = gates.shape[0]
    return torch.from_numpy(params.from_internal(f"{NAME}/kernel", gates.reshape(B, -1).numpy()))


@pytest.mark.parametrize("masked", [True, False])
def test_step_matches_oracle(masked):
    """lstm_ref.step == oracle.zoneout_lstm_step (float64, 1e-12), masks and the eval blend;
    the gates it returns are the oracle cell's activated [i j f o]."""
    from oracle import sat_oracle as O
    g = torch.Generator().manual_seed(3 + masked)
    B, U, I = 5, 6, 8
    x, c, h = _rand(g, B, I), _rand(g, B, U), _rand(g, B, U)
    w, b = _rand(g, I + U, 4 * U, scale=0.3), _rand(g, 4 * U, scale=0.3)
    mc = (torch.rand(B, U, generator=g) < 0.7).to(F64) if masked else None
    mh = (torch.rand(B, U, generator=g) < 0.7).to(F64) if masked else None
    zc, zh = 0.1, 0.25
    o_raw, o_c, o_h = O.zoneout_lstm_step(x, c, h, w, b, zc, zh, mc, mh)
    Wi, bi = _internal(w, b)
    rows = torch.cat([x, h], dim=-1)
    h_raw, c_out, h_out, gates, pre = R.step(bi, rows, Wi, c, h, mc, mh, zc, zh)
    for got, ref in ((h_raw, o_raw), (c_out, o_c), (h_out, o_h)):
        assert float((got - ref).abs().max()) <= 1e-12
    z = rows @ w + b
    assert float((_gates_tf(pre) - z).abs().max()) <= 1e-12
    i, j, f, o = torch.chunk(z, 4, dim=-1)
    ref_g = torch.cat([torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)], -1)
    assert float((_gates_tf(gates) - ref_g).abs().max()) <= 1e-12
    # the hoisted form (xproj = x @ W_x + b per row, recurrent rows only) is the same cell
    xproj = (x @ Wi[:I].reshape(I, -1)).view(B, U, 4) + bi
    again = R.step(xproj, h, Wi[I:], c, h, mc, mh, zc, zh)
    assert float((again[0] - o_raw).abs().max()) <= 1e-12
    # an invalid row copies its state, outputs 0
    valid = torch.tensor([True, False, True, False, True])
    hv, cv, h2v, gv, _ = R.step(bi, rows, Wi, c, h, mc, mh, zc, zh, valid=valid)
    assert torch.equal(hv[1], torch.zeros(U, dtype=F64)) and torch.equal(gv[3], torch.zeros(U, 4, dtype=F64))
    assert torch.equal(cv[1], c[1]) and torch.equal(h2v[3], h[3])
    assert torch.equal(hv[0], h_raw[0]) and torch.equal(cv[2], c_out[2])


@pytest.mark.parametrize("masked", [True, False])
def test_bilstm_matches_oracle(masked):
    """lstm_ref.bilstm == oracle.lstm_sequence forward and reverse, ragged lengths (one full row,
    one of length 1), masks and the eval blend, to 1e-12; state rows follow SatEncLstmFwd."""
    from oracle import sat_oracle as O
    g = torch.Generator().manual_seed(11 + masked)
    B, N, U, I = 4, 7, 5, 6
    x = _rand(g, B, N, I)
    lengths = torch.tensor([N, 1, 4, 6])
    zc, zh = 0.1, 0.2
    ws = [(_rand(g, I + U, 4 * U, scale=0.3), _rand(g, 4 * U, scale=0.3)) for _ in range(2)]
    masks = None
    if masked:
        masks = tuple((torch.rand(N, B, U, generator=g) < 0.6).to(F64) for _ in range(4))
    outs = [O.lstm_sequence(x, lengths, w, b, zc, zh, None if masks is None else masks[2 * d],
                            None if masks is None else masks[2 * d + 1], reverse=bool(d))
            for d, (w, b) in enumerate(ws)]
    Xs, Wr = [], []
    for w, b in ws:
        Wi, bi = _internal(w, b)
        Xs.append(((x.reshape(B * N, I) @ Wi[:I].reshape(I, -1)).view(B, N, U, 4) + bi).reshape(B, N, 4 * U))
        Wr.append(Wi[I:])
    H, CS, HS, G = R.bilstm(Xs[0], Xs[1], Wr[0], Wr[1], lengths, masks, zc, zh)
    assert H.shape == (B, N, 2 * U) and CS[0].shape == (N + 1, B, U) and G[1].shape == (N, B, U, 4)
    assert float((H - torch.cat(outs, dim=-1)).abs().max()) <= 1e-12
    for b_, L in enumerate(lengths.tolist()):
        assert torch.equal(H[b_, L:], torch.zeros(N - L, 2 * U, dtype=F64))
        assert torch.equal(G[0][L:, b_], torch.zeros(N - L, U, 4, dtype=F64))
        # frozen states past the length (forward), untouched before the first valid step (backward)
        assert torch.equal(HS[0][L + 1:, b_], HS[0][L, b_].expand(N - L, -1))
        assert torch.equal(CS[1][L:, b_], torch.zeros(N + 1 - L, U, dtype=F64))
    assert torch.equal(CS[0][0], torch.zeros(B, U, dtype=F64))
    # the forward state history is the oracle's recurrence: row n + 1 = state after step n
    c = h = torch.zeros(B, U, dtype=F64)
    w, b = ws[0]
    for n in range(N):
        v = (n < lengths).to(F64).unsqueeze(1)
        _, c2, h2 = O.zoneout_lstm_step(x[:, n], c, h, w, b, zc, zh,
                                        None if masks is None else masks[0][n],
                                        None if masks is None else masks[1][n])
        c, h = v * c2 + (1 - v) * c, v * h2 + (1 - v) * h
        assert float((CS[0][n + 1] - c).abs().max()) <= 1e-12
        assert float((HS[0][n + 1] - h).abs().max()) <= 1e-12


@pytest.mark.parametrize("masked,hoff,with_dq", [(True, 0, False), (False, 0, False),
                                                 (True, 8, True), (False, 8, True)])
def test_step_bwd_matches_autograd(masked, hoff, with_dq):
    """lstm_ref.step_bwd chained over 5 steps with its carries == autograd of lstm_ref.step
    (1e-10): masks / eval blend, one row that runs out at step 2 (invalid steps), a query-gradient
    (dq) term on the raw output, hoff > 0.  Checks every step's gate gradients and the gradients
    of the initial state recovered from the last carries."""
    g = torch.Generator().manual_seed(5 + 2 * masked + hoff)
    T, B, U, D = 5, 3, 4, 8
    K = hoff + U
    W = _rand(g, K, U, 4, scale=0.5)
    xin = _rand(g, T, B, hoff)
    xproj = [_rand(g, B, U, 4).requires_grad_(True) for _ in range(T)]
    c0, h0 = _rand(g, B, U).requires_grad_(True), _rand(g, B, U).requires_grad_(True)
    lengths = torch.tensor([T, 2, T])
    zc, zh = 0.1, 0.3
    mcs = [(torch.rand(B, U, generator=g) < 0.6).to(F64) if masked else None for _ in range(T)]
    mhs = [(torch.rand(B, U, generator=g) < 0.6).to(F64) if masked else None for _ in range(T)]
    DY = _rand(g, T, B, U)
    DQ = _rand(g, T, B, D)
    wq = _rand(g, U, D)
    c, h = c0, h0
    loss = 0.0
    gates, cprev = [], []
    for t in range(T):
        rows = torch.cat([xin[t], h], dim=-1)
        cprev.append(c.detach())
        h_raw, c, h, gt, _ = R.step(xproj[t], rows, W, c, h, mcs[t], mhs[t], zc, zh,
                                    valid=t < lengths)
        gates.append(gt.detach())
        loss = loss + (h_raw * DY[t]).sum()
        if with_dq:
            loss = loss + ((h_raw @ wq) * DQ[t]).sum()
    loss.backward()
    dgn = dhc = dcc = None
    for t in reversed(range(T)):
        dgn, dhc, dcc = R.step_bwd(W, hoff, gates[t], cprev[t], dgn, None, DY[t],
                                   [(DQ[t], wq)] if with_dq else None, dhc, dcc, mcs[t], mhs[t],
                                   zc, zh, valid=t < lengths)
        assert float((dgn - xproj[t].grad).abs().max()) <= 1e-10
        if t < 2:
            assert float(dgn[1].abs().max()) > 0.0
        else:
            assert torch.equal(dgn[1], torch.zeros(U, 4, dtype=F64))
    dh0 = dhc + torch.einsum("bvg,uvg->bu", dgn, W[hoff:])
    assert float((dh0 - h0.grad).abs().max()) <= 1e-10
    assert float((dcc - c0.grad).abs().max()) <= 1e-10
    # the precomputed recurrent product is the same step (dgates_next then unused)
    rec = torch.einsum("bvg,uvg->bu", dgn, W[hoff:])
    a = R.step_bwd(W, hoff, gates[0], cprev[0], dgn, None, DY[0], None, dhc, dcc, mcs[0], mhs[0], zc, zh)
    b = R.step_bwd(W, hoff, gates[0], cprev[0], None, rec, DY[0], None, dhc, dcc, mcs[0], mhs[0], zc, zh)
    for x, y in zip(a, b):
        assert float((x - y).abs().max()) <= 1e-14


def test_bilstm_gate_gradients_are_step_bwd():
    """autograd(sum H . DY) w.r.t. X_fw / X_bw (the GPU test's gate-gradient reference) equals
    lstm_ref.step_bwd run in each direction's reverse order (1e-10), zeros at invalid steps."""
    g = torch.Generator().manual_seed(23)
    B, N, U = 3, 6, 4
    lengths = torch.tensor([N, 1, 4])
    X = [_rand(g, B, N, 4 * U).requires_grad_(True) for _ in range(2)]
    W = [_rand(g, U, U, 4, scale=0.5) for _ in range(2)]
    masks = tuple((torch.rand(N, B, U, generator=g) < 0.6).to(F64) for _ in range(4))
    DY = _rand(g, B, N, 2 * U)
    H, CS, HS, G = R.bilstm(X[0], X[1], W[0], W[1], lengths, masks, 0.1, 0.1)
    (H * DY).sum().backward()
    for d in range(2):
        dgn = dhc = dcc = None
        for n in (range(N) if d else range(N - 1, -1, -1)):
            cp = CS[d][n + 1 if d else n].detach()
            dgn, dhc, dcc = R.step_bwd(W[d], 0, G[d][n].detach(), cp, dgn, None,
                                       DY[:, n, d * U:(d + 1) * U], None, dhc, dcc,
                                       masks[2 * d][n], masks[2 * d + 1][n], 0.1, 0.1,
                                       valid=n < lengths)
            ref = X[d].grad[:, n].view(B, U, 4)
            assert float((dgn - ref).abs().max()) <= 1e-10
            for b_, L in enumerate(lengths.tolist()):
                if n >= L:
                    assert torch.equal(ref[b_], torch.zeros(U, 4, dtype=F64))


def _stack_case(g, T, B, U, masked):
    """Random decoder-stack operands in float64: hoisted X1, the three weights, a non-zero
    initial state, masks (or None) and a head gradient."""
    X1 = _rand(g, T, B, 4 * U)
    W1r, W2 = _rand(g, U, U, 4, scale=0.5), _rand(g, 2 * U, U, 4, scale=0.4)
    b2 = _rand(g, U, 4, scale=0.3)
    init = tuple(_rand(g, B, U, scale=0.5) for _ in range(4))
    masks = None
    if masked:
        masks = tuple((torch.rand(T, B, U, generator=g) < 0.6).to(F64) for _ in range(4))
    return X1, W1r, W2, b2, init, masks, _rand(g, T, B, U)


@pytest.mark.parametrize("masked", [True, False])
def test_decoder_stack_matches_oracle(masked):
    """lstm_ref.decoder_stack == a chain of oracle.zoneout_lstm_step calls wired as the oracle's
    decoder_loop wires lstm1 into lstm2 (lstm2's input is lstm1's RAW output), float64 to 1e-12:
    masks and the eval blend, a non-zero initial state, zc != zh.  State row t + 1 is the state
    after step t, row 0 the state given; the gates are the oracle cell's activated [i j f o]."""
    from oracle import sat_oracle as O
    g = torch.Generator().manual_seed(31 + masked)
    T, B, U, I = 6, 3, 5, 7
    zc, zh = 0.1, 0.15
    x = _rand(g, T, B, I)
    w1, b1 = _rand(g, I + U, 4 * U, scale=0.3), _rand(g, 4 * U, scale=0.3)
    w2, b2 = _rand(g, 2 * U, 4 * U, scale=0.3), _rand(g, 4 * U, scale=0.3)
    init = tuple(_rand(g, B, U, scale=0.5) for _ in range(4))
    masks = None
    if masked:
        masks = tuple((torch.rand(T, B, U, generator=g) < 0.6).to(F64) for _ in range(4))
    W1i, b1i = _internal(w1, b1)
    W2i, b2i = _internal(w2, b2)
    X1 = ((x.reshape(T * B, I) @ W1i[:I].reshape(I, -1)).view(T, B, U, 4) + b1i).reshape(T, B, 4 * U)
    H1RAW, C1S, H1S, G1, H2RAW, C2S, H2S, G2 = R.decoder_stack(X1, W1i[I:], W2i, b2i, init, masks,
                                                               zc, zh)
    assert H1RAW.shape == H2RAW.shape == (T, B, U) and G1.shape == G2.shape == (T, B, 4 * U)
    assert C1S.shape == H1S.shape == C2S.shape == H2S.shape == (T + 1, B, U)
    for got, ref in zip((C1S[0], H1S[0], C2S[0], H2S[0]), init):
        assert torch.equal(got, ref)
    cc1, hh1, cc2, hh2 = init
    for t in range(T):
        m = (None,) * 4 if masks is None else tuple(mk[t] for mk in masks)
        z1 = torch.cat([x[t], hh1], dim=-1) @ w1 + b1
        h1_out, cc1, hh1 = O.zoneout_lstm_step(x[t], cc1, hh1, w1, b1, zc, zh, m[0], m[1])
        z2 = torch.cat([h1_out, hh2], dim=-1) @ w2 + b2
        h2_out, cc2, hh2 = O.zoneout_lstm_step(h1_out, cc2, hh2, w2, b2, zc, zh, m[2], m[3])
        for got, ref in ((H1RAW[t], h1_out), (C1S[t + 1], cc1), (H1S[t + 1], hh1),
                         (H2RAW[t], h2_out), (C2S[t + 1], cc2), (H2S[t + 1], hh2)):
            assert float((got - ref).abs().max()) <= 1e-12
        for got, z in ((G1[t], z1), (G2[t], z2)):
            i, j, f, o = torch.chunk(z, 4, dim=-1)
            ref_g = torch.cat([torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0),
                               torch.sigmoid(o)], -1)
            assert float((_gates_tf(got) - ref_g).abs().max()) <= 1e-12
    # X2 = 0 changes nothing
    again = R.decoder_stack(X1, W1i[I:], W2i, b2i, init, masks, zc, zh,
                            X2=torch.zeros(T, B, 4 * U, dtype=F64))
    assert torch.equal(again[4], H2RAW) and torch.equal(again[7], G2)


@pytest.mark.parametrize("masked", [True, False])
def test_decoder_stack_gate_gradients_are_step_bwd(masked):
    """What the GPU test calls DG1 / DG2: autograd of sum(H2RAW . DH2) w.r.t. X1 and X2 equals a
    reverse loop of lstm_ref.step_bwd over both layers (1e-10) -- LSTM2 with dy = DH2[t] and its
    recurrent rows W2[U:], LSTM1 with dy = dgates2_t . W2[:U] (the gradient of its raw output
    through LSTM2's input rows) and its own recurrent product."""
    g = torch.Generator().manual_seed(41 + masked)
    T, B, U = 6, 3, 4
    zc, zh = 0.1, 0.15
    X1, W1r, W2, b2, init, masks, DH2 = _stack_case(g, T, B, U, masked)
    X1 = X1.requires_grad_(True)
    X2 = torch.zeros(T, B, 4 * U, dtype=F64, requires_grad=True)
    H1RAW, C1S, H1S, G1, H2RAW, C2S, H2S, G2 = R.decoder_stack(X1, W1r, W2, b2, init, masks, zc,
                                                               zh, X2=X2)
    (H2RAW * DH2).sum().backward()
    dg1 = dg2 = dh1 = dc1 = dh2 = dc2 = None
    for t in reversed(range(T)):
        m = (None,) * 4 if masks is None else tuple(mk[t] for mk in masks)
        dg2, dh2, dc2 = R.step_bwd(W2, U, G2[t].detach().view(B, U, 4), C2S[t].detach(), dg2, None,
                                   DH2[t], None, dh2, dc2, m[2], m[3], zc, zh)
        dy1 = torch.einsum("bvg,uvg->bu", dg2, W2[:U])
        dg1, dh1, dc1 = R.step_bwd(W1r, 0, G1[t].detach().view(B, U, 4), C1S[t].detach(), dg1, None,
                                   dy1, None, dh1, dc1, m[0], m[1], zc, zh)
        assert float((dg2.reshape(B, -1) - X2.grad[t]).abs().max()) <= 1e-10
        assert float((dg1.reshape(B, -1) - X1.grad[t]).abs().max()) <= 1e-10
        assert float(dg1.abs().max()) > 0.0 and float(dg2.abs().max()) > 0.0
