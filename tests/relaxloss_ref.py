"""Restatement of the reference's boundary label relaxation (--jointwtborder) for the tests:

  multihot()        RelaxedBoundaryLossToTensor.__call__, transforms/transforms.py:90-123: scipy's integer `shift` with
                    cval = C is an exact array shift, so channel c of a pixel is 1 iff a pixel of its (2b+1)^2 window has
                    label c, positions outside the image counting as the ignore channel C; a pixel whose own label is in
                    the strict list keeps its one-hot
  class_sets()      the two 64-bit words per pixel the kernels keep instead (bit c = channel c), as int64 [B,H,W,2]
  stats()           set entries per channel and the pixels without a real class, int64 [B,C+2]
  class_weights()   calculate_weights, loss/utils.py:165-177 in numpy float64, then torch.Tensor(): one rounding to fp32
  loss()            ImgWtLossSoftNLL.forward, loss/utils.py:179-231, in float64 torch with autograd.  For the classes of a
                    set log(max(soft_c, m_c * S)) = log S, so the term of a pixel is -q * (sum_{c in set} w_c) * log S;
                    q = sum over ALL images of the batch of 1 / border weight (the reference passes the whole [B,H,W]
                    tensor to every image's custom_nll, where it broadcasts)

tests/test_relaxloss_cpu.py holds this file to the golden data recorded from the real reference."""
import numpy as np
import torch


def multihot(labels, C, ignore, border=1, strict=None):
    """labels: integer array [B,H,W] -> uint8 [B,C+1,H,W]"""
    lab = np.asarray(labels).astype(np.int64)
    B, H, W = lab.shape
    lab = np.where((lab == ignore) | (lab < 0) | (lab >= C), C, lab)
    pad = np.full((B, H + 2 * border, W + 2 * border), C, dtype=np.int64)
    pad[:, border:border + H, border:border + W] = lab
    out = np.zeros((B, C + 1, H, W), dtype=np.uint8)
    bi, yi, xi = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    for dy in range(2 * border + 1):
        for dx in range(2 * border + 1):
            out[bi, pad[:, dy:dy + H, dx:dx + W], yi, xi] = 1
    if strict is not None:
        keep = np.isin(lab, [c for c in strict if 0 <= c < C])
        one = np.zeros_like(out)
        one[bi, lab, yi, xi] = 1
        out = np.where(keep[:, None], one, out)
    return out


def class_sets(mh):
    """uint8 [B,C+1,H,W] -> int64 [B,H,W,2] (the bit patterns of two unsigned 64-bit words)"""
    mh = np.asarray(mh) != 0
    B, C1, H, W = mh.shape
    words = np.zeros((B, H, W, 2), dtype=np.uint64)
    for c in range(C1):
        words[..., c // 64] |= mh[:, c].astype(np.uint64) << np.uint64(c % 64)
    return torch.from_numpy(words.view(np.int64).copy())


def stats(mh):
    """uint8 [B,C+1,H,W] -> int64 [B,C+2]: set entries per channel, then the pixels whose set holds no real class"""
    mh = np.asarray(mh) != 0
    counts = mh.sum(axis=(2, 3)).astype(np.int64)
    ign = (mh[:, :-1].sum(axis=1) == 0).sum(axis=(1, 2)).astype(np.int64)
    return torch.from_numpy(np.concatenate([counts, ign[:, None]], axis=1))


def class_weights(mh, upper_bound=1.0, batch_weights=False):
    """uint8 [B,C+1,H,W] -> fp32 [B,C]"""
    mh = (np.asarray(mh) != 0).astype(np.uint8)
    rows = []
    for i in range(mh.shape[0]):
        t = mh if batch_weights else mh[i]
        axes = (0, 2, 3) if batch_weights else (1, 2)
        hist = np.sum(t, axis=axes) * 1.0 / t.sum()
        hist = ((hist != 0) * upper_bound * (1 - hist)) + 1
        rows.append(torch.Tensor(hist[:-1]))
    return torch.stack(rows)


def loss(logits, mh, upper_bound=1.0, batch_weights=False):
    """logits [B,C,H,W] (any float type; float64 is used), mh uint8 [B,C+1,H,W] -> float64 scalar with autograd"""
    m = torch.from_numpy((np.asarray(mh)[:, :-1] != 0).astype(np.float64))
    B, C, H, W = m.shape
    w = class_weights(mh, upper_bound, batch_weights).double()
    bw = m.sum(1)
    ign = bw == 0
    q = (1.0 / torch.where(ign, torch.ones_like(bw), bw)).sum(0)
    logp = torch.log_softmax(logits.double(), dim=1)
    total = 0.0
    for i in range(B):
        # log S over the set, finite where the set is empty (those pixels are masked below)
        log_s = torch.logsumexp(torch.where(m[i] > 0, logp[i], torch.full_like(logp[i], -1e300)), dim=0)
        term = -q * (m[i] * w[i][:, None, None]).sum(0) * log_s
        term = torch.where(ign[i], torch.zeros_like(term), term)
        total = total + term.sum() / (H * W - int(ign[i].sum()) + 1)
    return total
