"""Plain-torch restatement of the zoneout LSTM kernels (csrc/lstm.hip, csrc/encoder_lstm.hip,
csrc/decoder_lstm_persistent.hip) in the kernels' own layout, dtype-generic (float64 for the
reference, float32 to measure what the number format alone costs).  Shared by
test_lstm_ref_cpu.py (which ties it to the oracle), test_lstm_gpu.py, test_encoder_lstm_gpu.py
and test_decoder_lstms_gpu.py.

Layout: weights [K][U][4], gates / gate gradients [B][U][4], gate order i, j, f, o, forget
bias 1.  Zoneout: masks (1 = take the new value) or, with ``mc is None``, the eval blend
(1 - z) new + z old.  A row with ``valid == False`` copies its state and emits h_raw = 0,
gates = 0 (bidirectional_dynamic_rnn's sequence_length).
"""
import torch


def _zeros_like_state(rows, U):
    return rows.new_zeros(rows.shape[0], U)


def step(xb, rows, W, c_prev, h_prev, mc, mh, zc, zh, valid=None):
    """One forward step.  ``xb``: the hoisted input projection [B][U][4], a bias [U][4] or None;
    ``rows`` [B][K]: the already concatenated [rin | rin1 | rin2]; ``W`` [K][U][4];
    ``c_prev`` / ``h_prev`` [B][U] or None (zeros); ``valid`` [B] bool or None (all valid).
    Returns (h_raw, c_out, h_out, gates, pre)."""
    U = W.shape[1]
    pre = torch.einsum("bk,kug->bug", rows, W)
    if xb is not None:
        pre = pre + xb
    cp = _zeros_like_state(rows, U) if c_prev is None else c_prev
    hp = _zeros_like_state(rows, U) if h_prev is None else h_prev
    gi = torch.sigmoid(pre[..., 0])
    gj = torch.tanh(pre[..., 1])
    gf = torch.sigmoid(pre[..., 2] + 1.0)
    go = torch.sigmoid(pre[..., 3])
    cn = gf * cp + gi * gj
    hn = go * torch.tanh(cn)
    if mc is not None:
        c2 = mc * cn + (1.0 - mc) * cp
        h2 = mh * hn + (1.0 - mh) * hp
    else:
        c2 = (1.0 - zc) * cn + zc * cp
        h2 = (1.0 - zh) * hn + zh * hp
    gates = torch.stack([gi, gj, gf, go], dim=-1)
    if valid is not None:
        v = valid.to(torch.bool).unsqueeze(1)
        zero = torch.zeros_like(hn)
        hn = torch.where(v, hn, zero)
        c2 = torch.where(v, c2, cp)
        h2 = torch.where(v, h2, hp)
        gates = torch.where(v.unsqueeze(-1), gates, torch.zeros_like(gates))
    return hn, c2, h2, gates, pre


def step_bwd(W, hoff, gates, c_prev, dgates_next, rec, dy, dqs, dh_carry, dc_carry, mc, mh, zc,
             zh, valid=None):
    """One reverse step, by hand from the comment on SatLstmBwd (include/sat_abi.h):

        dL/dh_t  = dh_carry + dgates_next . W[hoff + u]      (or + rec, the product precomputed)
        dL/dh'_t = dy + sum_parts dq . wq[u] + m_h dL/dh_t
        dL/dc'_t = m_c dL/dc_t + dL/dh'_t o (1 - tanh(c')^2)

    ``gates`` [B][U][4] activated; ``dgates_next`` [B][U][4] or None; ``rec`` [B][U] or None;
    ``dqs``: list of (dq [B][D] -- already summed over its partials, wq [U][D]).  ``dgates`` are
    the gradients of the gate PRE-activations.  Returns (dgates, dh_carry_out, dc_carry_out);
    an invalid row passes its carries through and has dgates = 0."""
    B, U, _ = gates.shape
    z = gates.new_zeros(B, U)
    dh_t = z if dh_carry is None else dh_carry
    if rec is not None:
        dh_t = dh_t + rec
    elif dgates_next is not None:
        dh_t = dh_t + torch.einsum("bvg,uvg->bu", dgates_next, W[hoff:hoff + U])
    dc_t = z if dc_carry is None else dc_carry
    q = z
    for dq, wq in dqs or ():
        q = q + dq @ wq.T
    cp = z if c_prev is None else c_prev
    if mc is None:
        mc, mh = 1.0 - zc, 1.0 - zh
    gi, gj, gf, go = gates.unbind(-1)
    tc = torch.tanh(gf * cp + gi * gj)
    dhn = (z if dy is None else dy) + q + mh * dh_t
    dcn = mc * dc_t + dhn * go * (1.0 - tc * tc)
    dg = torch.stack([dcn * gj * gi * (1.0 - gi), dcn * gi * (1.0 - gj * gj),
                      dcn * cp * gf * (1.0 - gf), dhn * tc * go * (1.0 - go)], dim=-1)
    dc_out = dcn * gf + (1.0 - mc) * dc_t
    dh_out = (1.0 - mh) * dh_t
    if valid is not None:
        v = valid.to(torch.bool).unsqueeze(1)
        dg = torch.where(v.unsqueeze(-1), dg, torch.zeros_like(dg))
        dc_out = torch.where(v, dc_out, dc_t)
        dh_out = torch.where(v, dh_out, dh_t)
    return dg, dh_out, dc_out


def bilstm(X_fw, X_bw, W_fw, W_bw, lengths, masks, zc, zh, init=None):
    """Both directions over all N steps, in SatEncLstmFwd's layout.

    ``X_*`` [B][N][4U] (hoisted input projections + bias, gate-interleaved), ``W_*`` [U][U][4]
    (or [U][4U]), ``lengths`` [B] int64, ``masks`` None (eval blend) or
    (mc_fw, mh_fw, mc_bw, mh_bw) each [N][B][U], ``init`` None (zeros) or
    (c_fw, h_fw, c_bw, h_bw) each [B][U].

    Returns H [B][N][2U], CS (fw, bw), HS (fw, bw) each [N+1][B][U], G (fw, bw) each
    [N][B][U][4].  State rows: the forward direction reads row 0 and writes row n + 1 at step n;
    the backward direction reads row N and writes row n at step n.  Differentiable."""
    B, N, G4 = X_fw.shape
    U = G4 // 4
    Hs, CSs, HSs, Gs = [], [], [], []
    for d, (X, W) in enumerate(((X_fw, W_fw), (X_bw, W_bw))):
        W = W.reshape(U, U, 4)
        c = X.new_zeros(B, U) if init is None else init[2 * d]
        h = X.new_zeros(B, U) if init is None else init[2 * d + 1]
        cs, hs, g, out = [None] * (N + 1), [None] * (N + 1), [None] * N, [None] * N
        r0 = N if d else 0
        cs[r0], hs[r0] = c, h
        for n in (range(N - 1, -1, -1) if d else range(N)):
            mc = None if masks is None else masks[2 * d][n]
            mh = None if masks is None else masks[2 * d + 1][n]
            out[n], c, h, g[n], _ = step(X[:, n].reshape(B, U, 4), h, W, c, h, mc, mh, zc, zh,
                                         valid=n < lengths)
            nx = n if d else n + 1
            cs[nx], hs[nx] = c, h
        Hs.append(torch.stack(out, dim=1))
        CSs.append(torch.stack(cs))
        HSs.append(torch.stack(hs))
        Gs.append(torch.stack(g))
    return torch.cat(Hs, dim=-1), tuple(CSs), tuple(HSs), tuple(Gs)


def decoder_stack(X1, W1r, W2, b2, init, masks, zc, zh, X2=None):
    """The decoder's two stacked ZoneoutLSTM layers over all T steps, in SatDecLstmFwd's layout.

    ``X1`` [T][B][4U] (LSTM1's hoisted input projection + bias, gate-interleaved), ``W1r``
    [U][U][4] (LSTM1's recurrent rows), ``W2`` [2U][U][4] (LSTM2's input rows, then its recurrent
    rows), ``b2`` [U][4] (or [4U]), ``init`` = (c1, h1, c2, h2) each [B][U], ``masks`` None (eval
    blend) or (m1c, m1h, m2c, m2h) each [T][B][U], ``X2`` optional [T][B][4U] added to LSTM2's
    pre-activations (pass zeros: it exists so that autograd yields LSTM2's gate gradients).

    Per step LSTM1 takes X1[t] and rows h1_{t-1}; LSTM2 takes b2 (+ X2[t]) and rows
    [h1'_t | h2_{t-1}] -- LSTM1's RAW output, not its zoned-out state.

    Returns H1RAW [T][B][U], C1S, H1S [T+1][B][U] (row 0 = the initial state), G1 [T][B][4U],
    then H2RAW, C2S, H2S, G2 likewise.  Differentiable."""
    T, B, G4 = X1.shape
    U = G4 // 4
    W1r = W1r.reshape(U, U, 4)
    W2 = W2.reshape(2 * U, U, 4)
    b2 = b2.reshape(U, 4)
    c1, h1, c2, h2 = init
    raw1, cs1, hs1, g1 = [], [c1], [h1], []
    raw2, cs2, hs2, g2 = [], [c2], [h2], []
    for t in range(T):
        m = (None,) * 4 if masks is None else tuple(mk[t] for mk in masks)
        r1, c1, h1, gt1, _ = step(X1[t].reshape(B, U, 4), h1, W1r, c1, h1, m[0], m[1], zc, zh)
        xb2 = b2 if X2 is None else b2 + X2[t].reshape(B, U, 4)
        r2, c2, h2, gt2, _ = step(xb2, torch.cat([r1, h2], dim=-1), W2, c2, h2, m[2], m[3], zc, zh)
        raw1.append(r1), cs1.append(c1), hs1.append(h1), g1.append(gt1.reshape(B, G4))
        raw2.append(r2), cs2.append(c2), hs2.append(h2), g2.append(gt2.reshape(B, G4))
    st = torch.stack
    return st(raw1), st(cs1), st(hs1), st(g1), st(raw2), st(cs2), st(hs2), st(g2)
