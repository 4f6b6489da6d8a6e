"""The boundary F-score as a composition of torch operators on the device: per class two boolean boundary maps (seg2bmap's
shifted XORs), F.conv2d with the disk, four sums.  The yardstick of the full-size test of tests/test_fboundary_gpu.py
(held to tests/fboundary_ref.py there, where that is cheap) and the `torch` column of tools/fboundarybench.py: one
definition for both."""
import torch
import torch.nn.functional as F


def bmap(seg):
    e, s, se = torch.zeros_like(seg), torch.zeros_like(seg), torch.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def disk_conv(x, disk, r, rows=128):
    """F.conv2d(x, disk, padding=r) of [N,1,H,W] 0/1 maps, taken in strips of `rows` output rows by torch's own
    im2col + GEMM convolution (the vendor convolution library switched off for the call: it would build a kernel for
    every new filter size at first use, seconds each); a strip bounds the im2col buffer to (2r+1)^2 * rows * W floats.
    Sums of at most (2r+1)^2 ones: exact in fp32 in any order."""
    xp = F.pad(x, (0, 0, r, r))
    with torch.backends.cudnn.flags(enabled=False):
        return torch.cat([F.conv2d(xp[:, :, y0:y0 + rows + 2 * r], disk, padding=(0, r))
                          for y0 in range(0, x.shape[2], rows)], 2)


def torch_composition(pred, gt, C, ignore, r):
    """The counts from torch operators on the device: per-class boundary maps, F.conv2d with the disk."""
    B, H, W = pred.shape
    ign = gt == ignore
    ax = torch.arange(-r, r + 1, device=pred.device)
    disk = ((ax[:, None] ** 2 + ax[None, :] ** 2) <= r * r).float()[None, None]
    out = torch.zeros((B, C, 4), dtype=torch.int64, device=pred.device)

    for i in range(B):
        for c in range(C):
            fg_b, gt_b = bmap((pred[i] == c) & ~ign[i]), bmap((gt[i] == c) & ~ign[i])
            dil = disk_conv(torch.stack([fg_b, gt_b]).float()[:, None], disk, r)[:, 0] > 0.5
            out[i, c, 0], out[i, c, 1] = fg_b.sum(), gt_b.sum()
            out[i, c, 2], out[i, c, 3] = (fg_b & dil[1]).sum(), (gt_b & dil[0]).sum()
    return out
