"""Float64 references of the per-RoI recognition kernels (test infrastructure; a helper module, not a conftest).

Each function is the reference project's formula written out on explicit weights - no state dict, no module - and computes
on the CPU in `dtype` (torch.float64; torch.float32 gives the plain fp32 evaluation of the same formulas, whose distance to
the float64 result is what the GPU tests derive their bounds from):

  gc_attention       MultiAspectGCAttention minus its out-conv (glass/modeling/fusion/fusion_modules.py:91-143) on the
                     channel-interleaved [R, 256, 512] slab csrc/fusion_attention.hip takes
  lstm_direction /   nn.LSTM (gate order i, f, g, o; zero initial state) from the gate pre-activations
  bilstm             (glass/modeling/recognition/recognizer_encoder.py:118-144): csrc/bilstm.hip, csrc/recurrent_persistent.hip
  decoder_step       AttentionUnit + DecoderUnit (glass/modeling/recognition/prediction_aster.py:247-266, 291-302):
                     glass_attention_decode_step
  greedy_decode      AttentionRecognitionHead.sample (prediction_aster.py:63-99), one call of the reference per image:
                     glass_attention_decode / glass_attention_decode_persistent

tests/test_recognition_ref.py pins every one of them to the fp32 oracle (oracle/glass_cpu.py) without a GPU."""
import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ fusion attention
def gc_attention(x, w_mask, b_mask, w1, b1, ln_g, ln_b, w2, b2, heads=8, eps=1e-5, dtype=F64):
    """x [R, HW, C]: channel 2i = local i, 2i+1 = global i (the reference's x[:, order], channels last).  Head h owns the
    channels [h C/heads, (h+1) C/heads): softmax over the HW positions of conv_mask (one weight row w_mask [C/heads] shared by
    the heads, b_mask [1]), context = sum_pos x softmax; channel_add = conv1x1 (w1 [P, C], b1) -> LayerNorm over P (biased
    variance, eps; ln_g, ln_b [P]) -> ReLU -> conv1x1 (w2 [C, P], b2); the result is x + channel_add, broadcast over positions.
    -> (out [R, HW, C], dict of the intermediates: mask logits [R, HW, heads], hid [R, P] before the LayerNorm)"""
    x, w_mask, b_mask, w1, b1, ln_g, ln_b, w2, b2 = (t.to(dtype) for t in (x, w_mask, b_mask, w1, b1, ln_g, ln_b, w2, b2))
    R, HW, C = x.shape
    cp = C // heads
    xh = x.reshape(R, HW, heads, cp)
    logit = (xh * w_mask.reshape(1, 1, 1, cp)).sum(-1) + b_mask.reshape(())
    a = torch.softmax(logit, dim=1)
    ctx = (xh * a.unsqueeze(-1)).sum(1).reshape(R, C)
    hid = ctx @ w1.reshape(-1, C).t() + b1
    mean = hid.mean(1, keepdim=True)
    var = ((hid - mean) ** 2).mean(1, keepdim=True)
    y = torch.relu((hid - mean) / torch.sqrt(var + eps) * ln_g.reshape(1, -1) + ln_b.reshape(1, -1))
    t = y @ w2.reshape(C, -1).t() + b2
    return x + t.unsqueeze(1), {"logit": logit, "hid": hid}


# ------------------------------------------------------------------------------------------------ BiLSTM recurrence
def lstm_direction(xg, w_hh, reverse, dtype=F64):
    """xg [R, T, 4 Hd]: x_t W_ih^T + b_ih + b_hh of ONE direction; w_hh [4 Hd, Hd] -> h [R, T, Hd] (and the last cell state)"""
    xg, w_hh = xg.to(dtype), w_hh.to(dtype)
    R, T, _ = xg.shape
    Hd = w_hh.shape[1]
    h = xg.new_zeros((R, Hd))
    c = xg.new_zeros((R, Hd))
    out = xg.new_zeros((R, T, Hd))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        i, f, g, o = (xg[:, t] + h @ w_hh.t()).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[:, t] = h
    return out, c


def bilstm(xg, w_hh, dtype=F64):
    """xg [R, T, 2, 4 Hd] (direction-major, then gate-major), w_hh [2, 4 Hd, Hd] -> [R, T, 2 Hd] (forward | backward)"""
    return torch.cat([lstm_direction(xg[:, :, d], w_hh[d], bool(d), dtype)[0] for d in (0, 1)], dim=2)


# ------------------------------------------------------------------------------------------------ attention decoder
def make_decoder_plain(C, seed, D=256, fc_scale=0.5, temperature=1.0):
    """a decoder's weights as torch stores them (float32, CPU) for any class count: sW [D, D] sEmbed, xW [D, D] xEmbed, wW [D] /
    wB [1] wEmbed, emb [C, D], GRU w_ih [3D, 2D] (input = [embedding | context]) / w_hh [3D, D], fcW [C, D]; the scales are
    those of the project's synthetic checkpoint"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)
    return {"sW": r(D, D) / 16, "sB": r(D) * 0.1, "xW": r(D, D) / 16, "xB": r(D) * 0.1, "wW": r(D) * 0.25, "wB": r(1) * 0.1,
            "emb": r(C, D), "w_ih": r(3 * D, 2 * D) / 16, "w_hh": r(3 * D, D) / 16, "b_ih": r(3 * D) * 0.1, "b_hh": r(3 * D) * 0.1,
            "fcW": r(C, D) * fc_scale, "fcB": r(C) * 0.1, "temperature": float(temperature)}


def plain_from_state_dict(sd, prefix):
    """the same dict from a checkpoint's decoder (`prefix` ends in "recognizer.decoder.")"""
    f = lambda k: sd[prefix + k].float()
    return {"sW": f("attention_unit.sEmbed.weight"), "sB": f("attention_unit.sEmbed.bias"), "xW": f("attention_unit.xEmbed.weight"),
            "xB": f("attention_unit.xEmbed.bias"), "wW": f("attention_unit.wEmbed.weight").reshape(-1),
            "wB": f("attention_unit.wEmbed.bias").reshape(-1), "emb": f("tgt_embedding.weight"), "w_ih": f("gru.weight_ih_l0"),
            "w_hh": f("gru.weight_hh_l0"), "b_ih": f("gru.bias_ih_l0"), "b_hh": f("gru.bias_hh_l0"), "fcW": f("fc.weight"),
            "fcB": f("fc.bias"), "temperature": float(sd[prefix + "temperature"].reshape(-1)[0]) if prefix + "temperature" in sd else 1.0}


def pack_kblocked(w):
    """packed[k / 4][row][k % 4] = W[row][k] (include/glass_hip.h)"""
    rows, K = w.shape
    return w.reshape(rows, K // 4, 4).permute(1, 0, 2).contiguous()


def pack_decoder(plain, device):
    """the dict ASTER_V2.import_weights builds from a checkpoint (k-blocked sW / fcW, row-major GRU matrices, sW_rm, emb_gi in
    float64 stored as float32) - without xW / xB: the tests hand the kernels xproj itself"""
    D = plain["w_hh"].shape[1]
    w = {k: plain[k].float().contiguous() for k in ("sB", "wW", "wB", "emb", "w_ih", "w_hh", "b_ih", "b_hh", "fcB")}
    w["sW"] = pack_kblocked(plain["sW"].float())
    w["fcW"] = pack_kblocked(plain["fcW"].float())
    w["sW_rm"] = plain["sW"].float().contiguous()
    w["emb_gi"] = (plain["emb"].double() @ plain["w_ih"][:, :D].double().t() + plain["b_ih"].double()).float().contiguous()
    w = {k: v.to(device) for k, v in w.items()}
    w["temperature"] = float(plain["temperature"])
    return w


def xproj_of(x, plain):
    """xEmbed(x), rounded once to float32: the step-invariant input both the kernels and the references are given"""
    return (x.double() @ plain["xW"].double().t() + plain["xB"].double()).float()


def decoder_step(x, xproj, h, y_prev, W, dtype=F64):
    """x, xproj [R, T, D], h [R, D], y_prev [R] ints (clamped to [0, C), as the C ABI says) -> (logits, probs, h_out):
    alpha = softmax_t(wEmbed(tanh(sEmbed(h) + xproj))), context = alpha . x, GRU cell on [emb[y_prev] | context], logits =
    fc(h_out) * temperature"""
    c = lambda k: W[k].to(dtype)
    x, xproj, h = x.to(dtype), xproj.to(dtype), h.to(dtype)
    C = W["fcW"].shape[0]
    y = y_prev.long().clamp(0, C - 1)
    sp = h @ c("sW").t() + c("sB")
    e = torch.tanh(sp.unsqueeze(1) + xproj) @ c("wW").reshape(-1) + c("wB").reshape(())
    alpha = torch.softmax(e, dim=1)
    ctx = (alpha.unsqueeze(-1) * x).sum(1)
    gi = torch.cat([c("emb")[y], ctx], 1) @ c("w_ih").t() + c("b_ih")
    gh = h @ c("w_hh").t() + c("b_hh")
    i_r, i_z, i_n = gi.chunk(3, 1)
    h_r, h_z, h_n = gh.chunk(3, 1)
    r = torch.sigmoid(i_r + h_r)
    z = torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    h_out = (1 - z) * n + z * h
    logits = (h_out @ c("fcW").t() + c("fcB")) * W["temperature"]
    return logits, torch.softmax(logits, dim=1), h_out


TIE_EPS = 1e-12      # float64 probabilities closer than this to the maximum count as equal to it (constructed exact ties)


def greedy_decode(x, xproj, W, roi_image, max_len, eos, dtype=F64):
    """The greedy decoder with the reference's early break, which is global over ONE call of the reference = one image:
    roi_image [R] ints.  The first maximum wins (torch.max); classes within TIE_EPS of the maximum are one tie group.
    -> dict: probs [R, max_len, C] (rows after an image's break are zero), pred [R, max_len] (-1 after the break), live
    [R, max_len] bool, gap [R, max_len] = maximum minus the best class OUTSIDE its tie group (inf where there is none), ties
    [R, max_len] = size of the tie group"""
    R, T, D = x.shape
    C = W["fcW"].shape[0]
    probs = torch.zeros((R, max_len, C), dtype=dtype)
    pred = torch.full((R, max_len), -1, dtype=torch.long)
    live = torch.zeros((R, max_len), dtype=torch.bool)
    gap = torch.full((R, max_len), float("inf"), dtype=dtype)
    ties = torch.zeros((R, max_len), dtype=torch.long)
    roi_image = torch.as_tensor(roi_image).long()
    for img in roi_image.unique().tolist():
        idx = (roi_image == img).nonzero().squeeze(1)
        xi, xpi = x[idx], xproj[idx]
        h = torch.zeros((len(idx), D), dtype=dtype)
        y = torch.zeros((len(idx),), dtype=torch.long)
        dones = torch.zeros((len(idx),), dtype=torch.bool)
        for i in range(max_len):
            _, p, h = decoder_step(xi, xpi, h, y, W, dtype)
            top = p.max(1, keepdim=True).values
            tied = p >= top - TIE_EPS
            y = torch.where(tied, torch.arange(C).unsqueeze(0), torch.full((1, 1), C)).min(1).values
            rest = torch.where(tied, torch.full_like(p, -float("inf")), p).max(1).values
            probs[idx, i], pred[idx, i], live[idx, i] = p, y, True
            gap[idx, i], ties[idx, i] = top.squeeze(1) - rest, tied.sum(1)
            dones |= y == eos
            if bool(dones.all()):
                break
    return {"probs": probs, "pred": pred, "live": live, "gap": gap, "ties": ties}
