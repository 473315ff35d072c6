"""numpy mirror of the index rule of idiff_dihedral_rows (include/idiff.h), element by element, and the torch expression it is stated
against.  Shared by tests/test_self_ensemble_cpu.py and tests/test_self_ensemble_gpu.py."""
import numpy as np


def dihedral_ref(src, k):
    """src [..., H, W] -> the image under code k, by the header's rule: y1 = bit1 ? H-1-y : y, x1 = bit2 ? W-1-x : x,
    out[y, x] = bit0 ? src[x1, y1] : src[y1, x1].  The output has the input's H x W, so a transposing code needs H == W."""
    src = np.asarray(src)
    H, W = src.shape[-2:]
    if k & 1 and H != W:
        raise ValueError("a transposing code needs a square image")
    out = np.empty_like(src)
    for y in range(H):
        y1 = H - 1 - y if k & 2 else y
        for x in range(W):
            x1 = W - 1 - x if k & 4 else x
            out[..., y, x] = src[..., x1, y1] if k & 1 else src[..., y1, x1]
    return out


def dihedral_rows_ref(src, codes, S, in_rep, R=None):
    """src [R / in_rep, C, H, W] -> [R, C, H, W]: row r is input row r // in_rep under code codes[(r % S) % len(codes)]"""
    src = np.asarray(src)
    R = src.shape[0] * in_rep if R is None else R
    return np.stack([dihedral_ref(src[r // in_rep], codes[(r % S) % len(codes)]) for r in range(R)])


def dihedral_torch(x, k):
    """the torch expression of the contract: transpose if bit 0, then flip H if bit 1, then flip W if bit 2"""
    t = x.transpose(-1, -2) if k & 1 else x
    if k & 2:
        t = t.flip(-2)
    if k & 4:
        t = t.flip(-1)
    return t.contiguous()
